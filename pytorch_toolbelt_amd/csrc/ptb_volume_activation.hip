// ptb_volume_activation.hip -- sigmoid / softmax of the model's logits inside the 3-D mirror de-augmentation and the three tile merges
// (mirror_volume_deaugment, VolumeMerger.integrate_batch / integrate_batch_deaugment, plain and deferred; activation=), gfx950 / MI355X.
//
// A(y) = (y.float() * temperature).sigmoid() | .softmax(dim=1) is applied to every view of every tile in registers, where the planar
// and channels-last kernels (ptb_volume_tta.hip, ptb_volume_channels_last.hip, ptb_volume_bands.hip) only widen the logit: each call here
// means its namesake there on A(y), a float32 tensor that never exists.  So the source counts as float32 (no rounding of the reduced value
// to a half source type), and the order of every sum is the namesake's: views in view order through red_pre / red_post, tile * window
// rounded and added in integration order, the quotient by __fdiv_rn.
//
// Work division: softmax couples the C values of one (tile, view, voxel), so the channels are RESIDENT instead of walked by the grid.
//   * dense source, on the 4-voxel grid: a lane owns 4 consecutive x and up to 8 channels (16- / 8-byte loads per channel plane);
//   * dense source otherwise, and softmax over 9..16 channels: a lane owns one voxel and up to 16 channels;
//   * channels-last source: a lane owns one voxel and its (up to 16) contiguous channels, 16- / 8-byte loads when C % 4 == 0 and the
//     tiles are aligned, element loads otherwise.
// Sigmoid walks the channels in groups of that capacity through the same code (no limit on C); softmax needs C in one group (C <= 16).
// The gather walks the covering tiles in the outer loop and the views inside, with a per-channel blend accumulator: every logit is read
// once.  Activation, reduction, view masks, C and all extents are wave-uniform run-time values; source dtype, layout, lane width and the
// result kind are the template axes.  No LDS, no atomics, no scratch.
#include <cmath>

#include "ptb_activation_device.h"
#include "ptb_crop_device.h"
#include "ptb_dispatch.h"
#include "ptb_mirror_device.h"
#include "ptb_volume_device.h"

namespace ptb {

namespace {

constexpr int ACT_BLOCK = 256;
constexpr int ACT_GRID_X = 8192;  // workgroups over the units of one tile (grid-stride beyond), as the planar mirror kernels
constexpr long long ACT_MAX_PLANE = 0x7fffffffLL - (long long)ACT_GRID_X * ACT_BLOCK;  // voxels of one [D, H, W] plane: int unit indices
constexpr int ACT_MAX_SOFTMAX_C = 16;

// voxels per lane and resident channels of an instance
template <bool CL, bool VEC>
constexpr int act_pix() { return (!CL && VEC) ? 4 : 1; }
template <bool CL, bool VEC>
constexpr int act_creg() { return act_pix<CL, VEC>() == 4 ? 8 : 16; }

// v[c][..] <- channels c0 + c (c < nc) of the PIX voxels that view `m` puts at output (z, y, x ..) of a [C, D, H, W] (dense) or
// [D, H, W, C] (channels-last) block whose first element is element `off0` of `src`; a W-flipped run is reversed in registers.  The
// channels from nc to the end of the last group of four repeat channel nc - 1 (a valid address, an L1 hit; see activate)
template <int LD, bool CL, bool VEC, int CREG, int PIX>
__device__ __forceinline__ void act_load(float (&v)[CREG][PIX], const void* __restrict__ src, long long off0, int m, int z, int y, int x, int D,
                                         int H, int W, int C, int c0, int nc) {
    const long long vox = mirror_src<PIX>(m, z, y, x, D, H, W);
    if constexpr (CL) {
        const long long o = off0 + vox * C + c0;
        if constexpr (VEC) {
#pragma unroll
            for (int c = 0; c < CREG; c += 4) {
                if (c < nc) {
                    const float4 t = ld4<LD>(static_cast<const float*>(src), o + c);
                    v[c][0] = t.x; v[c + 1][0] = t.y; v[c + 2][0] = t.z; v[c + 3][0] = t.w;
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < CREG; g += 4) {
                if (g < nc) {
#pragma unroll
                    for (int c = g; c < g + 4; ++c) v[c][0] = widen<ld_dtype<LD>()>(src, o + min(c, nc - 1));
                }
            }
        }
    } else {
        const long long plane = (long long)D * H * W;
#pragma unroll
        for (int g = 0; g < CREG; g += 4) {
            if (g < nc) {
#pragma unroll
                for (int c = g; c < g + 4; ++c) {
                    const long long o = off0 + (c0 + min(c, nc - 1)) * plane + vox;
                    if constexpr (PIX == 4) {
                        float4 t = ld4<LD>(static_cast<const float*>(src), o);
                        if (m & 1) t = rev4(t);
                        v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
                    } else {
                        v[c][0] = widen<ld_dtype<LD>()>(src, o);
                    }
                }
            }
        }
    }
}

// view k of a tile is loaded: r <- r + pre(A(v)) (k = 0: r <- pre(A(v)))
template <int CREG, int PIX>
__device__ __forceinline__ void act_fold(float (&r)[CREG][PIX], float (&v)[CREG][PIX], int k, int nc, int op, int act, float temp) {
    activate(v, nc, act, temp);
    act_red_pre(v, nc, op);
    act_each(r, nc, [&](float s, int c, int j) { return k ? __fadd_rn(s, v[c][j]) : v[c][j]; });
}

// r[c][..] = post(sum_v pre(A(unflip_v(view v)))) for the channels c0 + c (c < nc) of one tile: mirror_reduce_voxels with the activation
// between the load and red_pre.  `off0` = element offset of view 0 of the tile, `view_stride` = elements between its views.
template <int LD, bool CL, bool VEC, int CREG, int PIX>
__device__ __forceinline__ void act_reduce_views(float (&r)[CREG][PIX], const void* __restrict__ src, long long off0, long long view_stride, int nv,
                                                 int masks, int op, float divisor, int act, float temp, int z, int y, int x, int D, int H, int W, int C,
                                                 int c0, int nc) {
#pragma unroll
    for (int c = 0; c < CREG; ++c) {
#pragma unroll
        for (int j = 0; j < PIX; ++j) r[c][j] = 0.f;
    }
#pragma unroll 1
    for (int k = 0; k < nv; ++k) {
        float v[CREG][PIX];
        act_load<LD, CL, VEC>(v, src, off0 + k * view_stride, (masks >> (3 * k)) & 7, z, y, x, D, H, W, C, c0, nc);
        act_fold(r, v, k, nc, op, act, temp);
    }
    act_red_post(r, nc, op, divisor);
}

// unit u of a [D, H, W] box of PIX-runs (x fastest, then y, then z; xq runs per row) -> (z, y, x)
template <int PIX>
__device__ __forceinline__ void act_unit(int u, int xq, int H, int& z, int& y, int& x) {
    const int row = u / xq;
    x = (u - row * xq) * PIX;
    z = row / H;
    y = row - z * H;
}

template <int PIX>
__device__ __forceinline__ void act_weight(float (&w)[PIX], const float* __restrict__ weight, long long off) {
    if constexpr (PIX == 4) {
        const float4 t = *reinterpret_cast<const float4*>(weight + off);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    } else {
        w[0] = weight[off];
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ de-augment + reduce
// out[b] = reduce_v(pre(A(unflip_v(src[v * B + b])))), dense float32 [B, C, D, H, W].  blockIdx.y walks the tiles b.
template <int LD, bool CL, bool VEC>
__global__ __launch_bounds__(ACT_BLOCK) void act_reduce_kernel(const MirrorArgs a, const int act, const float temp) {
    constexpr int PIX = act_pix<CL, VEC>(), CREG = act_creg<CL, VEC>();
    const int xq = a.W / PIX;
    const int units = a.D * a.H * xq;
    const long long plane = (long long)a.D * a.H * a.W;
    const long long tile_elems = a.C * plane;
    float* __restrict__ dst = static_cast<float*>(a.dst);
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        for (int u = blockIdx.x * ACT_BLOCK + threadIdx.x; u < units; u += gridDim.x * ACT_BLOCK) {
            int z, y, x;
            act_unit<PIX>(u, xq, a.H, z, y, x);
            const long long o = b * tile_elems + ((long long)z * a.H + y) * a.W + x;
            for (int c0 = 0; c0 < a.C; c0 += CREG) {
                const int nc = min(CREG, a.C - c0);
                float r[CREG][PIX];
                act_reduce_views<LD, CL, VEC>(r, a.src, b * tile_elems, a.view_stride, a.nv, a.masks, a.op, a.divisor, act, temp, z, y, x, a.D, a.H,
                                              a.W, a.C, c0, nc);
#pragma unroll
                for (int c = 0; c < CREG; ++c) {
                    if (c < nc) {
                        float* p = dst + o + (c0 + c) * plane;
                        if constexpr (PIX == 4) out_store4(p, make_float4(r[c][0], r[c][1], r[c][2], r[c][3]));
                        else p[0] = r[c][0];
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ fused blend
// One tile per launch, like volume_mirror_accumulate_kernel: a tile never overlaps itself, so a launch owns its accumulator region and
// stream order gives the sequential fp32 order.  volume[:, roi] += t * weight (product rounded, then added); norm[roi] += weight.
template <int LD, bool CL, bool VEC>
__global__ __launch_bounds__(ACT_BLOCK) void act_accum_kernel(const MirrorAccArgs a, const int act, const float temp) {
    constexpr int PIX = act_pix<CL, VEC>(), CREG = act_creg<CL, VEC>();
    const int xq = a.w / PIX;
    const int units = a.d * a.h * xq;
    const long long vplane = (long long)a.D * a.H * a.W;
    for (int u = blockIdx.x * ACT_BLOCK + threadIdx.x; u < units; u += gridDim.x * ACT_BLOCK) {
        int z, y, x;
        act_unit<PIX>(u, xq, a.h, z, y, x);
        const long long toff = ((long long)z * a.h + y) * a.w + x;
        const long long voff = ((long long)(a.z0 + z) * a.H + (a.y0 + y)) * a.W + a.x0 + x;
        float w[PIX];
        act_weight<PIX>(w, a.weight, toff);
        for (int c0 = 0; c0 < a.C; c0 += CREG) {
            const int nc = min(CREG, a.C - c0);
            float r[CREG][PIX];
            act_reduce_views<LD, CL, VEC>(r, a.tiles, a.tile_off, a.view_stride, a.nv, a.masks, a.op, a.divisor, act, temp, z, y, x, a.d, a.h, a.w,
                                          a.C, c0, nc);
#pragma unroll
            for (int c = 0; c < CREG; ++c) {
                if (c < nc) {
                    float* vp = a.volume + (c0 + c) * vplane + voff;
                    if constexpr (PIX == 4) {
                        float4 v = *reinterpret_cast<float4*>(vp);
                        v.x = __fadd_rn(v.x, __fmul_rn(r[c][0], w[0])); v.y = __fadd_rn(v.y, __fmul_rn(r[c][1], w[1]));
                        v.z = __fadd_rn(v.z, __fmul_rn(r[c][2], w[2])); v.w = __fadd_rn(v.w, __fmul_rn(r[c][3], w[3]));
                        *reinterpret_cast<float4*>(vp) = v;
                    } else {
                        vp[0] = __fadd_rn(vp[0], __fmul_rn(r[c][0], w[0]));
                    }
                }
            }
        }
        float* np = a.norm + voff;
        if constexpr (PIX == 4) {
            float4 n = *reinterpret_cast<float4*>(np);
            n.x = __fadd_rn(n.x, w[0]); n.y = __fadd_rn(n.y, w[1]); n.z = __fadd_rn(n.z, w[2]); n.w = __fadd_rn(n.w, w[3]);
            *reinterpret_cast<float4*>(np) = n;
        } else {
            np[0] = __fadd_rn(np[0], w[0]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ deferred slab merge
namespace {

// q[m] <- q[m + s] (s in 0..3) with compile-time register indices
template <typename T, int PIX>
__device__ __forceinline__ void act_shift(T (&q)[PIX], int s) {
    if constexpr (PIX == 4) {
        if (s == 1) { q[0] = q[1]; q[1] = q[2]; q[2] = q[3]; }
        else if (s == 2) { q[0] = q[2]; q[1] = q[3]; }
        else if (s == 3) { q[0] = q[3]; }
    }
}

// Channel c of a run is ready: store it (cast and layout of ptb_merge_crop.hip), or fold it into the running argmax (first maximum
// wins; NaN counts as the maximum, like numpy / torch argmax) -- emit_channel of ptb_volume_bands.hip
template <int KIND, int PIX>
__device__ __forceinline__ void act_emit(const VolArgs& a, const VolPos& p, int c, float (&q)[PIX], float (&best)[PIX], int (&arg)[PIX]) {
    if constexpr (vb_argmax<KIND>()) {
#pragma unroll
        for (int m = 0; m < PIX; ++m) {
            const bool take = c == 0 ? true : (q[m] > best[m] || (q[m] != q[m] && best[m] == best[m]));
            best[m] = take ? q[m] : best[m];
            arg[m] = take ? c : arg[m];
        }
    } else {
        act_shift(q, p.first);
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < PIX; ++m) o[m] = q[m];
        if (a.layout == 0 || a.C == 1) {
            store_out<KIND>(a.out, c * ((long long)a.OD * a.OH * a.OW) + p.vox, o, p.cnt);
        } else {
#pragma unroll
            for (int m = 0; m < PIX; ++m) {
                if (m < p.cnt) {
                    const float one[4] = {o[m], 0.f, 0.f, 0.f};
                    store_out<KIND>(a.out, (p.vox + m) * a.C + c, one, 1);
                }
            }
        }
    }
}

template <int KIND, int PIX>
__device__ __forceinline__ void act_emit_argmax(const VolArgs& a, const VolPos& p, int (&arg)[PIX]) {
    if constexpr (vb_argmax<KIND>()) {
        act_shift(arg, p.first);
        if constexpr (KIND == PTB_CROP_ARGMAX_U8) {
            uint8_t b[4] = {0, 0, 0, 0};
#pragma unroll
            for (int m = 0; m < PIX; ++m) b[m] = (uint8_t)arg[m];
            store_u8x4(static_cast<uint8_t*>(a.out) + p.vox, b, p.cnt);
        } else {
            long long* o = static_cast<long long*>(a.out) + p.vox;
#pragma unroll
            for (int m = 0; m < PIX; ++m)
                if (m < p.cnt) o[m] = arg[m];
        }
    }
}

}  // namespace

// One workgroup per work item of the plan's table (volume_gather_kernel).  Sums start from the item's `zero` (+0 the compiler cannot
// fold), so a cell nobody covers divides 0 by 0 like the plain merge, with no path of its own.
template <int LD, bool CL, bool VEC, int KIND>
__global__ __launch_bounds__(VB_BLOCK) void act_gather_kernel(const VolArgs a, const VolTiles t, const int act, const float temp) {
    constexpr int PIX = act_pix<CL, VEC>(), CREG = act_creg<CL, VEC>();
    const VolItem* it = a.items + blockIdx.x;
    const int ntiles = it->ntiles;
    const int nx = it->nx, ny = it->ny, nz = it->nz, x0 = it->x0, y0 = it->y0, z0 = it->z0;
    const int xq = (nx + PIX - 1) / PIX;
    const int units = nz * ny * xq;
    const float zero = __int_as_float(it->zero);
    for (int u = threadIdx.x; u < units; u += VB_BLOCK) {
        int dz, dy, dx;
        act_unit<PIX>(u, xq, ny, dz, dy, dx);
        VolPos p = vol_pos(a, z0 + dz, y0 + dy, x0 + dx, min(PIX, nx - dx));
        if (p.cnt <= 0) continue;                       // the 4-aligned hull of the window in x: nothing to store
        float n[PIX];
#pragma unroll
        for (int j = 0; j < PIX; ++j) n[j] = zero;
        for (int k = 0; k < ntiles; ++k) {
            const unsigned long long cv = it->cover[k];
            float w[PIX];
            act_weight<PIX>(w, a.weight, (((int)(cv >> 48) + dz) * a.h + (int)((cv >> 32) & 0xffffu) + dy) * a.w + (int)((cv >> 16) & 0xffffu) + dx);
#pragma unroll
            for (int j = 0; j < PIX; ++j) n[j] = __fadd_rn(n[j], w[j]);
        }
        float best[PIX];
        int arg[PIX];
#pragma unroll
        for (int j = 0; j < PIX; ++j) { best[j] = 0.f; arg[j] = 0; }
        for (int c0 = 0; c0 < a.C; c0 += CREG) {
            const int nc = min(CREG, a.C - c0);
            float s[CREG][PIX];
#pragma unroll
            for (int c = 0; c < CREG; ++c) {
#pragma unroll
                for (int j = 0; j < PIX; ++j) s[c][j] = zero;
            }
#pragma unroll 1
            for (int k = 0; k < ntiles; ++k) {
                const unsigned long long cv = it->cover[k];
                const int slot = (int)(cv & 0xffffu);
                const int tz = (int)(cv >> 48) + dz, ty = (int)((cv >> 32) & 0xffffu) + dy, tx = (int)((cv >> 16) & 0xffffu) + dx;
                float r[CREG][PIX];
                act_reduce_views<LD, CL, VEC>(r, t.src[slot], 0, t.vs[slot], a.nv, a.masks, a.op, a.divisor, act, temp, tz, ty, tx, a.d, a.h, a.w,
                                              a.C, c0, nc);
                float w[PIX];
                act_weight<PIX>(w, a.weight, (tz * a.h + ty) * a.w + tx);
                act_each(s, nc, [&](float acc, int c, int j) { return __fadd_rn(acc, __fmul_rn(r[c][j], w[j])); });
            }
#pragma unroll
            for (int c = 0; c < CREG; ++c) {
                if (c < nc) {
                    float q[PIX];
#pragma unroll
                    for (int j = 0; j < PIX; ++j) q[j] = __fdiv_rn(s[c][j], n[j]);
                    act_emit<KIND, PIX>(a, p, c0 + c, q, best, arg);
                }
            }
        }
        act_emit_argmax<KIND, PIX>(a, p, arg);
    }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {

int act_pack_masks(int nviews, const int* masks, int& packed) {
    if (nviews < 1 || nviews > MAX_VIEWS || !masks) return PTB_EINVAL;
    packed = 0;
    for (int k = 0; k < nviews; ++k) {
        if (masks[k] < 0 || masks[k] > 7) return PTB_EINVAL;
        packed |= masks[k] << (3 * k);
    }
    return PTB_OK;
}

bool act_code_ok(int activation, float temperature) {
    return activation >= PTB_ACT_NONE && activation <= PTB_ACT_SOFTMAX && std::isfinite(temperature);
}

bool act_aligned_run(const void* p, int dtype) {  // 4 elements per lane: 16 B of fp32, 8 B of fp16 / bf16
    return (reinterpret_cast<uintptr_t>(p) & (dtype == PTB_F32 ? 15u : 7u)) == 0;
}

// dense: the 4-voxel lanes hold 8 channels, which softmax needs at once; channels-last: four channels per load
bool act_vec(bool src_cl, bool geom_ok, int activation, int C) {
    if (g_force_scalar || !geom_ok) return false;
    return src_cl ? C % 4 == 0 : (activation != PTB_ACT_SOFTMAX || C <= 8);
}

dim3 act_grid(long long units, long long tiles) {
    const long long gx = (units + ACT_BLOCK - 1) / ACT_BLOCK;
    return dim3((unsigned)(gx < ACT_GRID_X ? gx : ACT_GRID_X), (unsigned)(tiles < 65535 ? tiles : 65535));
}

// source dtype x layout x lane width: 12 instances
template <class F>
void with_act_instance(int dtype, bool src_cl, bool vec, F&& f) {
    with_src_dtype(dtype, [&](auto ld) { with_bool(src_cl, [&](auto cl) { with_bool(vec, [&](auto v) { f(ld, cl, v); }); }); });
}

}  // namespace

void act_launch_gather(const VolArgs& a, const VolTiles& t, int n_tiles, int dtype, bool src_cl, bool dense_vec, int kind, int n_items,
                       int activation, float temperature, hipStream_t s) {
    bool geom = dense_vec;
    if (src_cl) {
        geom = true;
        for (int k = 0; k < n_tiles; ++k) geom = geom && act_aligned_run(t.src[k], dtype) && t.vs[k] % 4 == 0;
    }
    const bool vec = act_vec(src_cl, geom, activation, a.C);
    const dim3 grid((unsigned)n_items), block(VB_BLOCK);
    with_act_instance(dtype, src_cl, vec, [&](auto ld, auto cl, auto v) { with_crop_kind(kind, [&](auto k) {
        hipLaunchKernelGGL((act_gather_kernel<ld(), cl(), v(), k()>), grid, block, 0, s, a, t, activation, temperature); }); });
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_volume_mirror_reduce_act(const void* src, int dtype, float* dst, int nviews, const int* masks, int reduction, int B, int C,
                                            int D, int H, int W, int activation, float temperature, ptb_stream_t stream) {
    const bool src_cl = (dtype & PTB_SRC_CHANNELS_LAST) != 0;
    dtype &= ~PTB_SRC_CHANNELS_LAST;
    if (!src || !dst || B < 0 || C < 1 || D < 1 || H < 1 || W < 1) return PTB_EINVAL;
    if (dtype < PTB_F32 || dtype > PTB_BF16 || reduction < PTB_RED_SUM || reduction > PTB_RED_LOG1P) return PTB_EINVAL;
    if (!act_code_ok(activation, temperature)) return PTB_EINVAL;
    int packed;
    if (int rc = act_pack_masks(nviews, masks, packed)) return rc;
    if (activation == PTB_ACT_SOFTMAX && C > ACT_MAX_SOFTMAX_C) return PTB_EUNSUPPORTED;
    if ((long long)D * H * W > ACT_MAX_PLANE) return PTB_EUNSUPPORTED;
    if (B == 0) return PTB_OK;
    MirrorArgs a{};
    a.src = src; a.dst = dst;
    a.B = B; a.C = C; a.D = D; a.H = H; a.W = W;
    a.nv = nviews; a.masks = packed;
    a.view_stride = (long long)B * C * D * H * W;
    a.op = reduction;
    a.divisor = reduction == PTB_RED_SUM ? 1.0f : (float)nviews;
    const bool geom = src_cl ? act_aligned_run(src, dtype) : (W % 4 == 0 && act_aligned_run(src, dtype) && aligned16(dst));
    const bool vec = act_vec(src_cl, geom, activation, C);
    const dim3 grid = act_grid((long long)D * H * (!src_cl && vec ? W / 4 : W), B);
    hipStream_t s = (hipStream_t)stream;
    with_act_instance(dtype, src_cl, vec, [&](auto ld, auto cl, auto v) {
        hipLaunchKernelGGL((act_reduce_kernel<ld(), cl(), v()>), grid, dim3(ACT_BLOCK), 0, s, a, activation, temperature); });
    return check_launch();
}

extern "C" int ptb_volume_mirror_accumulate_act(float* volume, float* norm, const float* weight, const void* tiles, int in_dtype, int nviews,
                                                const int* masks, int reduction, const int64_t* zs, const int64_t* ys, const int64_t* xs, int B,
                                                int C, int d, int h, int w, int D, int H, int W, int activation, float temperature,
                                                ptb_stream_t stream) {
    if (!volume || !norm || !weight || !tiles || !zs || !ys || !xs) return PTB_EINVAL;
    if (B < 0 || C < 1 || d < 1 || h < 1 || w < 1 || D < 1 || H < 1 || W < 1) return PTB_EINVAL;
    const bool src_cl = (in_dtype & PTB_SRC_CHANNELS_LAST) != 0;
    in_dtype &= ~PTB_SRC_CHANNELS_LAST;
    if (in_dtype < PTB_F32 || in_dtype > PTB_BF16 || reduction < PTB_RED_SUM || reduction > PTB_RED_LOG1P) return PTB_EINVAL;
    if (!act_code_ok(activation, temperature)) return PTB_EINVAL;
    int packed;
    if (int rc = act_pack_masks(nviews, masks, packed)) return rc;
    for (int b = 0; b < B; ++b)
        if (zs[b] < 0 || ys[b] < 0 || xs[b] < 0 || zs[b] + d > D || ys[b] + h > H || xs[b] + w > W) return PTB_EBOUNDS;
    if (activation == PTB_ACT_SOFTMAX && C > ACT_MAX_SOFTMAX_C) return PTB_EUNSUPPORTED;
    if ((long long)d * h * w > ACT_MAX_PLANE) return PTB_EUNSUPPORTED;
    if (B == 0) return PTB_OK;
    MirrorAccArgs a{};
    a.volume = volume; a.norm = norm; a.weight = weight; a.tiles = tiles;
    a.view_stride = (long long)B * C * d * h * w;
    a.C = C; a.d = d; a.h = h; a.w = w; a.D = D; a.H = H; a.W = W;
    a.nv = nviews; a.masks = packed; a.op = reduction;
    a.divisor = reduction == PTB_RED_SUM ? 1.0f : (float)nviews;
    const long long tile_elems = (long long)C * d * h * w;
    // channels-last lanes own one voxel (nothing but the source is read in runs); dense 4-voxel lanes need everything on the 4-voxel grid
    const bool base = src_cl ? act_aligned_run(tiles, in_dtype)
                             : (w % 4 == 0 && W % 4 == 0 && aligned16(volume) && aligned16(norm) && aligned16(weight) && act_aligned_run(tiles, in_dtype));
    hipStream_t s = (hipStream_t)stream;
    for (int b = 0; b < B; ++b) {
        a.tile_off = (long long)b * tile_elems;
        a.z0 = (int)zs[b]; a.y0 = (int)ys[b]; a.x0 = (int)xs[b];
        const bool vec = act_vec(src_cl, base && (src_cl || a.x0 % 4 == 0), activation, C);
        const dim3 grid = act_grid((long long)d * h * (!src_cl && vec ? w / 4 : w), 1);
        with_act_instance(in_dtype, src_cl, vec, [&](auto ld, auto cl, auto v) {
            hipLaunchKernelGGL((act_accum_kernel<ld(), cl(), v()>), grid, dim3(ACT_BLOCK), 0, s, a, activation, temperature); });
        if (int rc = check_launch()) return rc;
    }
    return PTB_OK;
}
