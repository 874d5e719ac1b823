// ptb_volume_tta.hip -- mirror test-time augmentation of the 3-D tiled-inference loop (inference/tta_3d.py):
//
//   * ptb_volume_mirror: mirror_volume_augment (cat of x.flip(dims) over the views), and the un-flipped [V, B, ...] stack that
//     mirror_volume_deaugment hands to a callable reduction or returns for reduction=None.
//   * ptb_volume_mirror_reduce: mirror_volume_deaugment with a PTB_RED_* reduction.
//   * ptb_volume_mirror_accumulate: VolumeMerger.integrate_batch_deaugment -- un-flip, reduce and blend in one pass per tile.
//
// A view is a 3-bit mask: bit 0 flips W, bit 1 flips H, bit 2 flips D.  Flips are pure index reversals, so every kernel here is a
// streaming kernel with coalesced reads and writes: a lane handles 4 consecutive x of one output row; a D- or H-flip only changes the
// source row, a W-flip reads the mirrored 4-run and reverses it in registers.  W % 4 != 0 or an unaligned pointer takes the scalar
// (one x per lane) instances.  The split with views (ptb_volume_split_mirror) extends the split kernel of ptb_volume_edges.hip.
#include <type_traits>

#include "ptb_dispatch.h"
#include "ptb_mirror_device.h"
#include "ptb_volume_device.h"

namespace ptb {

constexpr int MIRROR_BLOCK = 256;
constexpr int MIRROR_GRID_X = 8192;  // workgroups per plane set (grid-stride beyond)
constexpr long long MIRROR_MAX_PLANE = 0x7fffffffLL - MIRROR_GRID_X * MIRROR_BLOCK;  // voxels of one [D, H, W] plane: int unit indices

// (ld_dtype, mirror_src, rev4 and the per-voxel de-augmentation mirror_reduce_voxels: ptb_mirror_device.h)

// (MirrorArgs, MirrorAccArgs: ptb_volume_device.h)

// (unit index inside one [D, H, W] plane of PIX-runs) -> (z, y, x)
template <int PIX>
__device__ __forceinline__ void unit_zyx(int u, int wq, int H, int& z, int& y, int& x) {
    const int row = u / wq;
    x = (u - row * wq) * PIX;
    z = row / H;
    y = row - z * H;
}

// dst[v * B + b] = flip_v(src[b]) (view_stride == 0: augment) or flip_v(src[v * B + b]) (the un-flipped stack).  ES = element size:
// the copy moves bits, so fp32 and fp16 / bf16 are the only two instances.  blockIdx.y walks the output planes (v, b, c).
template <int ES, int PIX>
__global__ __launch_bounds__(MIRROR_BLOCK) void volume_mirror_kernel(const MirrorArgs a) {
    typedef typename std::conditional<ES == 4, unsigned int, unsigned short>::type E;
    const int wq = a.W / PIX;
    const int units = a.D * a.H * wq;
    const long long plane = (long long)a.D * a.H * a.W;
    const int planes_out = a.nv * a.B * a.C;
    for (int p = blockIdx.y; p < planes_out; p += gridDim.y) {
        const int k = p / (a.B * a.C);                  // view of this output plane
        const int bc = p - k * (a.B * a.C);
        const int m = (a.masks >> (3 * k)) & 7;
        const E* src = static_cast<const E*>(a.src) + (a.view_stride ? k * a.view_stride : 0) + bc * plane;
        E* dst = static_cast<E*>(a.dst) + (long long)p * plane;
        for (int u = blockIdx.x * MIRROR_BLOCK + threadIdx.x; u < units; u += gridDim.x * MIRROR_BLOCK) {
            int z, y, x;
            unit_zyx<PIX>(u, wq, a.H, z, y, x);
            const long long so = mirror_src<PIX>(m, z, y, x, a.D, a.H, a.W);
            const long long o = ((long long)z * a.H + y) * a.W + x;
            if constexpr (PIX == 1) {
                dst[o] = src[so];
            } else if constexpr (ES == 4) {
                const float4 t = ld16<true>(reinterpret_cast<const float*>(src + so));
                out_store4(reinterpret_cast<float*>(dst + o), (m & 1) ? rev4(t) : t);
            } else {
                typedef unsigned short u4 __attribute__((ext_vector_type(4)));
                const u4 t = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src + so));
                const u4 r = (m & 1) ? u4{t.w, t.z, t.y, t.x} : t;
                __builtin_nontemporal_store(r, reinterpret_cast<u4*>(dst + o));
            }
        }
    }
}

// out[b] = reduce_v(unflip_v(src[v * B + b])) in the source type (fp16 / bf16 rounded to nearest even).
template <int LD, int OPK, int PIX>
__global__ __launch_bounds__(MIRROR_BLOCK) void volume_mirror_reduce_kernel(const MirrorArgs a) {
    const int wq = a.W / PIX;
    const int units = a.D * a.H * wq;
    const long long plane = (long long)a.D * a.H * a.W;
    const int planes_out = a.B * a.C;
    for (int p = blockIdx.y; p < planes_out; p += gridDim.y) {
        for (int u = blockIdx.x * MIRROR_BLOCK + threadIdx.x; u < units; u += gridDim.x * MIRROR_BLOCK) {
            int z, y, x;
            unit_zyx<PIX>(u, wq, a.H, z, y, x);
            const float4 r = mirror_reduce_voxels<LD, OPK, PIX>(a.src, p * plane, a.view_stride, a.nv, a.masks, a.op, a.divisor, z, y,
                                                                x, a.D, a.H, a.W);
            const long long o = p * plane + ((long long)z * a.H + y) * a.W + x;
            constexpr int OUT = ld_dtype<LD>();
            if constexpr (PIX == 4) {
                out_store4_as<OUT>(static_cast<float*>(a.dst), o, r);
            } else if constexpr (OUT == PTB_F32) {
                static_cast<float*>(a.dst)[o] = r.x;
            } else {
                static_cast<unsigned short*>(a.dst)[o] = half_bits<OUT>(r.x);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ fused blend
// One tile b per launch, like volume_accumulate_kernel (ptb_volume_edges.hip): a tile never overlaps itself, so a launch owns its
// accumulator region and stream order gives ptb_volume_accumulate's sequential fp32 order.  volume[:, roi] += t * weight with
// t = mirror_reduce_voxels(..) rounded to the source type (round_src1: what ptb_volume_mirror_reduce stores), product rounded, then
// added -- the same bits as ptb_volume_mirror_reduce followed by ptb_volume_accumulate.  blockIdx.y = channel.
template <int LD, int OPK, int PIX>
__global__ __launch_bounds__(MIRROR_BLOCK) void volume_mirror_accumulate_kernel(const MirrorAccArgs a) {
    const int wq = a.w / PIX;
    const int units = a.d * a.h * wq;
    const int c = blockIdx.y;
    const long long tplane = (long long)a.d * a.h * a.w, vplane = (long long)a.D * a.H * a.W;
    float* vol = a.volume + c * vplane;
    for (int u = blockIdx.x * MIRROR_BLOCK + threadIdx.x; u < units; u += gridDim.x * MIRROR_BLOCK) {
        int z, y, x;
        unit_zyx<PIX>(u, wq, a.h, z, y, x);
        const float4 r = mirror_reduce_voxels<LD, OPK, PIX>(a.tiles, a.tile_off + c * tplane, a.view_stride, a.nv, a.masks, a.op, a.divisor,
                                                            z, y, x, a.d, a.h, a.w);
        const long long toff = ((long long)z * a.h + y) * a.w + x;
        const long long voff = ((long long)(a.z0 + z) * a.H + (a.y0 + y)) * a.W + a.x0 + x;
        if constexpr (PIX == 4) {
            const float4 t = make_float4(round_src1<LD>(r.x), round_src1<LD>(r.y), round_src1<LD>(r.z), round_src1<LD>(r.w));
            const float4 w4 = *reinterpret_cast<const float4*>(a.weight + toff);
            float4* vp = reinterpret_cast<float4*>(vol + voff);
            float4 v = *vp;
            v.x = __fadd_rn(v.x, __fmul_rn(t.x, w4.x)); v.y = __fadd_rn(v.y, __fmul_rn(t.y, w4.y));
            v.z = __fadd_rn(v.z, __fmul_rn(t.z, w4.z)); v.w = __fadd_rn(v.w, __fmul_rn(t.w, w4.w));
            *vp = v;
            if (c == 0) {
                float4* np = reinterpret_cast<float4*>(a.norm + voff);
                float4 n = *np;
                n.x = __fadd_rn(n.x, w4.x); n.y = __fadd_rn(n.y, w4.y); n.z = __fadd_rn(n.z, w4.z); n.w = __fadd_rn(n.w, w4.w);
                *np = n;
            }
        } else {
            const float wv = a.weight[toff];
            vol[voff] = __fadd_rn(vol[voff], __fmul_rn(round_src1<LD>(r.x), wv));
            if (c == 0) a.norm[voff] = __fadd_rn(a.norm[voff], wv);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
static int pack_masks(int nviews, const int* masks, int& packed) {
    if (nviews < 1 || nviews > MAX_VIEWS || !masks) return PTB_EINVAL;
    packed = 0;
    for (int k = 0; k < nviews; ++k) {
        if (masks[k] < 0 || masks[k] > 7) return PTB_EINVAL;
        packed |= masks[k] << (3 * k);
    }
    return PTB_OK;
}

static bool aligned_run(const void* p, int dtype) {  // 4 elements per lane: 16 B of fp32, 8 B of fp16 / bf16
    return (reinterpret_cast<uintptr_t>(p) & (dtype == PTB_F32 ? 15u : 7u)) == 0;
}

static dim3 plane_grid(long long units, long long planes) {
    const long long gx = (units + MIRROR_BLOCK - 1) / MIRROR_BLOCK;
    return dim3((unsigned)(gx < MIRROR_GRID_X ? gx : MIRROR_GRID_X), (unsigned)(planes < 65535 ? planes : 65535));
}

// source dtype x (linear | non-linear reduction) x (4 voxels | 1 voxel per lane)
template <class F>
static void with_mirror_instance(int dtype, int op, bool vec, F&& f) {
    with_src_dtype(dtype, [&](auto ld) { with_reduction(op, [&](auto opk) { with_bool(vec, [&](auto v) {
        f(ld, opk, int_c<(v() ? 4 : 1)>{}); }); }); });
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_volume_mirror(const void* src, int dtype, void* dst, int nviews, const int* masks, int in_is_batch, int B, int C,
                                 int D, int H, int W, ptb_stream_t stream) {
    if (!src || !dst || B < 0 || C < 1 || D < 1 || H < 1 || W < 1) return PTB_EINVAL;
    if (dtype < PTB_F32 || dtype > PTB_BF16 || (in_is_batch != 0 && in_is_batch != 1)) return PTB_EINVAL;
    int packed;
    if (int rc = pack_masks(nviews, masks, packed)) return rc;
    if ((long long)D * H * W > MIRROR_MAX_PLANE || (long long)nviews * B * C > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    if (B == 0) return PTB_OK;
    MirrorArgs a{};
    a.src = src; a.dst = dst;
    a.B = B; a.C = C; a.D = D; a.H = H; a.W = W;
    a.nv = nviews; a.masks = packed;
    a.view_stride = in_is_batch ? 0 : (long long)B * C * D * H * W;
    const bool vec = !g_force_scalar && W % 4 == 0 && aligned_run(src, dtype) && aligned_run(dst, dtype);
    const dim3 grid = plane_grid((long long)D * H * (vec ? W / 4 : W), (long long)nviews * B * C);
    hipStream_t s = (hipStream_t)stream;
    with_bool(dtype == PTB_F32, [&](auto f32) { with_bool(vec, [&](auto v) {   // element bytes x elements per lane
        hipLaunchKernelGGL((volume_mirror_kernel<(f32() ? 4 : 2), (v() ? 4 : 1)>), grid, dim3(MIRROR_BLOCK), 0, s, a); }); });
    return check_launch();
}

extern "C" int ptb_volume_mirror_reduce(const void* src, int dtype, void* dst, int nviews, const int* masks, int reduction, int B,
                                        int C, int D, int H, int W, ptb_stream_t stream) {
    const bool src_cl = (dtype & PTB_SRC_CHANNELS_LAST) != 0;
    dtype &= ~PTB_SRC_CHANNELS_LAST;
    if (!src || !dst || B < 0 || C < 1 || D < 1 || H < 1 || W < 1) return PTB_EINVAL;
    if (dtype < PTB_F32 || dtype > PTB_BF16 || reduction < PTB_RED_SUM || reduction > PTB_RED_LOG1P) return PTB_EINVAL;
    int packed;
    if (int rc = pack_masks(nviews, masks, packed)) return rc;
    if ((long long)D * H * W > MIRROR_MAX_PLANE || (long long)B * C > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    if (B == 0) return PTB_OK;
    MirrorArgs a{};
    a.src = src; a.dst = dst;
    a.B = B; a.C = C; a.D = D; a.H = H; a.W = W;
    a.nv = nviews; a.masks = packed;
    a.view_stride = (long long)B * C * D * H * W;
    a.op = reduction;
    a.divisor = reduction == PTB_RED_SUM ? 1.0f : (float)nviews;
    hipStream_t s = (hipStream_t)stream;
    if (src_cl) {   // PTB_SRC_CHANNELS_LAST: one lane per output voxel over all channels, any shape
        cl3_launch_reduce(a, dtype, s);
        return check_launch();
    }
    const bool vec = !g_force_scalar && W % 4 == 0 && aligned_run(src, dtype) && aligned_run(dst, dtype);
    const dim3 grid = plane_grid((long long)D * H * (vec ? W / 4 : W), (long long)B * C);
    with_mirror_instance(dtype, reduction, vec, [&](auto ld, auto opk, auto pix) {
        hipLaunchKernelGGL((volume_mirror_reduce_kernel<ld(), opk(), pix()>), grid, dim3(MIRROR_BLOCK), 0, s, a); });
    return check_launch();
}

extern "C" int ptb_volume_mirror_accumulate(float* volume, float* norm, const float* weight, const void* tiles, int in_dtype, int nviews,
                                            const int* masks, int reduction, const int64_t* zs, const int64_t* ys, const int64_t* xs,
                                            int B, int C, int d, int h, int w, int D, int H, int W, ptb_stream_t stream) {
    if (!volume || !norm || !weight || !tiles || !zs || !ys || !xs) return PTB_EINVAL;
    if (B < 0 || C < 1 || d < 1 || h < 1 || w < 1 || D < 1 || H < 1 || W < 1) return PTB_EINVAL;
    const bool src_cl = (in_dtype & PTB_SRC_CHANNELS_LAST) != 0;
    in_dtype &= ~PTB_SRC_CHANNELS_LAST;
    if (in_dtype < PTB_F32 || in_dtype > PTB_BF16 || reduction < PTB_RED_SUM || reduction > PTB_RED_LOG1P) return PTB_EINVAL;
    int packed;
    if (int rc = pack_masks(nviews, masks, packed)) return rc;
    for (int b = 0; b < B; ++b)
        if (zs[b] < 0 || ys[b] < 0 || xs[b] < 0 || zs[b] + d > D || ys[b] + h > H || xs[b] + w > W) return PTB_EBOUNDS;
    if ((long long)d * h * w > MIRROR_MAX_PLANE || C > 65535) return PTB_EUNSUPPORTED;
    if (B == 0) return PTB_OK;
    MirrorAccArgs a{};
    a.volume = volume; a.norm = norm; a.weight = weight; a.tiles = tiles;
    a.view_stride = (long long)B * C * d * h * w;
    a.C = C; a.d = d; a.h = h; a.w = w; a.D = D; a.H = H; a.W = W;
    a.nv = nviews; a.masks = packed; a.op = reduction;
    a.divisor = reduction == PTB_RED_SUM ? 1.0f : (float)nviews;
    if (src_cl) {   // PTB_SRC_CHANNELS_LAST: one launch per tile as below, one lane per voxel over all channels
        const long long tile_elems = (long long)C * d * h * w;
        for (int b = 0; b < B; ++b) {
            a.tile_off = (long long)b * tile_elems;
            a.z0 = (int)zs[b]; a.y0 = (int)ys[b]; a.x0 = (int)xs[b];
            cl3_launch_accum(a, in_dtype, (hipStream_t)stream);
            if (int rc = check_launch()) return rc;
        }
        return PTB_OK;
    }
    const bool base_vec = !g_force_scalar && w % 4 == 0 && W % 4 == 0 && aligned16(volume) && aligned16(norm) && aligned16(weight) &&
                          aligned_run(tiles, in_dtype);
    hipStream_t s = (hipStream_t)stream;
    const long long tile_elems = (long long)C * d * h * w;
    for (int b = 0; b < B; ++b) {
        a.tile_off = (long long)b * tile_elems;
        a.z0 = (int)zs[b]; a.y0 = (int)ys[b]; a.x0 = (int)xs[b];
        const bool vec = base_vec && a.x0 % 4 == 0;
        const dim3 grid = plane_grid((long long)d * h * (vec ? w / 4 : w), C);
        with_mirror_instance(in_dtype, reduction, vec, [&](auto ld, auto opk, auto pix) {
            hipLaunchKernelGGL((volume_mirror_accumulate_kernel<ld(), opk(), pix()>), grid, dim3(MIRROR_BLOCK), 0, s, a); });
        if (int rc = check_launch()) return rc;
    }
    return PTB_OK;
}
