// ptb_merge_crop.hip -- the last step of the tiled-inference loop, on the device, for 2-D images and 3-D volumes:
//
//   * ptb_merge_crop: TileMerger.merge (tiles.py:345-346) + CHW -> HWC (np.moveaxis) + .astype(uint8) (truncating,
//     README.md:225) or argmax over channels + ImageSlicer.crop_to_orignal_size (tiles.py:271-280) in one pass that
//     writes only the cropped window (25-100 MB to download instead of the 419 MB padded fp32 map).
//   * ptb_volume_merge_crop: VolumeMerger.merge (volume / norm_mask, ptb_merge_div) + crop to VolumeSlicer.orignal_image_roi
//     [+ channels last] [+ cast | argmax over channels] in one pass that reads and writes only the cropped window.
//
// One kernel family serves both: a 2-D call is a 3-D one with D = OD = 1 and z0 = 0.  HBM-bound streaming kernels (no MFMA);
// each lane owns 4 consecutive output voxels of one row and reads them with 16-byte loads when the window is aligned.
#include "ptb_crop_device.h"
#include "ptb_dispatch.h"

namespace ptb {

struct CropArgs {
    const float* vol;   // [C, D, H, W] accumulator
    const float* norm;  // [D, H, W], or NULL: vol is already normalised (a uniform test skips the division)
    void* out;
    int C, D, H, W;
    int z0, y0, x0, OD, OH, OW;
};

// (cast_u8 and the store_* helpers of the PTB_CROP_* kinds: ptb_crop_device.h)

// nv (<= 4) consecutive source floats of one row; `vec` (uniform): the window is 16 B aligned in the accumulator
__device__ __forceinline__ void load_px4(const float* p, int nv, bool vec, float* o) {
    if (vec && nv == 4) {
        const float4 t = ld16<true>(p);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
        for (int m = 0; m < 4; ++m) o[m] = m < nv ? p[m] : 1.0f;
    }
}

// Output voxel group t (4 consecutive x of one output row) -> its source offset, output voxel offset and width
struct CropPos { long long src, dst; int nv; };
__device__ __forceinline__ CropPos crop_pos(const CropArgs& a, long long t, int groups_x) {
    const long long row = t / groups_x;   // output row (z, y) = z * OH + y
    const int x = (int)(t - row * groups_x) * 4;
    long long srow = (long long)a.z0 * a.H + a.y0 + row;   // its source row (z0 + z) * H + y0 + y ...
    if (a.OD > 1) srow += row / a.OH * (a.H - a.OH);        // ... (uniform: z == 0 for every 2-D call, which skips the division)
    CropPos p;
    p.src = srow * a.W + a.x0 + x;
    p.dst = row * a.OW + x;
    p.nv = min(4, a.OW - x);
    return p;
}

// channel c of the group's 4 voxels, divided by their norm n (ptb_merge_div / tiles.py:346: no eps clamp)
__device__ __forceinline__ void load_div(const CropArgs& a, int c, const CropPos& p, bool vec, const float* n, float* v) {
    load_px4(a.vol + c * ((long long)a.D * a.H * a.W) + p.src, p.nv, vec, v);
    if (a.norm) {
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = __fdiv_rn(v[m], n[m]);
    }
}

// element e = m * CT + c of a thread's contiguous channel-last run of 4 voxels x CT channels (store group g = elements 4g .. 4g+3)
template <int CT>
__device__ __forceinline__ float run_elem(const float (&v)[CT][4], int e) { return v[e % CT][e / CT]; }

// Channel-planar outputs ([C, OD, OH, OW]), channel-last ones with C == 1 (the same bytes) and argmax ([OD, OH, OW]):
// one pass over the channels with running state, any C.
template <int KIND>
__global__ __launch_bounds__(256) void crop_planar_kernel(const CropArgs a, bool vec) {
    const int groups_x = (a.OW + 3) / 4;
    const long long total = (long long)a.OD * a.OH * groups_x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long oplane = (long long)a.OD * a.OH * a.OW;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const CropPos p = crop_pos(a, t, groups_x);
        float n[4], v[4];
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int arg[4] = {0, 0, 0, 0};
        if (a.norm) load_px4(a.norm + p.src, p.nv, vec, n);
        for (int c = 0; c < a.C; ++c) {
            load_div(a, c, p, vec, n, v);
            if constexpr (KIND == PTB_CROP_ARGMAX_U8 || KIND == PTB_CROP_ARGMAX_I64) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {  // first maximum wins; NaN counts as the maximum (numpy / torch argmax)
                    const bool take = c == 0 ? true : (v[m] > best[m] || (v[m] != v[m] && best[m] == best[m]));
                    best[m] = take ? v[m] : best[m];
                    arg[m] = take ? c : arg[m];
                }
            } else {
                store_out<KIND>(a.out, c * oplane + p.dst, v, p.nv);
            }
        }
        if constexpr (KIND == PTB_CROP_ARGMAX_U8) {
            uint8_t b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) b[m] = (uint8_t)arg[m];
            store_u8x4(static_cast<uint8_t*>(a.out) + p.dst, b, p.nv);
        } else if constexpr (KIND == PTB_CROP_ARGMAX_I64) {
            long long* o = static_cast<long long*>(a.out) + p.dst;
            for (int m = 0; m < p.nv; ++m) o[m] = arg[m];
        }
    }
}

// Channel-last outputs ([OD, OH, OW, C]).  CT in 2..4: the CT channels of 4 voxels held in registers, so the thread's 4 * CT
// contiguous output elements leave as CT full-width stores.  CT == 0: any C, element by element (not a tuned path).
// fp32 with OW % 4 == 0 (`repack`): thread t's run starts at element 4 * CT * t of the output, i.e. the 256 threads of a
// workgroup own 256 * CT consecutive float4 -- but a lane's own CT float4 are adjacent, so storing them directly makes every
// store instruction hit 64 lanes x 16 B at a stride of 16 * CT B (measured 3.2 TB/s).  The runs are exchanged through LDS
// instead (lane writes float4 CT * tid + g, reads float4 256 * g + tid), so each store instruction covers 1 KiB contiguous.
template <int KIND, int CT>
__global__ __launch_bounds__(256) void crop_last_kernel(const CropArgs a, bool vec, bool repack) {
    const int groups_x = (a.OW + 3) / 4;
    const long long total = (long long)a.OD * a.OH * groups_x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    if constexpr (KIND == PTB_CROP_F32 && CT > 0) {
        if (repack) {
            __shared__ float4 xchg[256 * CT];
            for (long long t0 = (long long)blockIdx.x * blockDim.x; t0 < total; t0 += stride) {   // workgroup-uniform trip count
                const long long t = t0 + threadIdx.x;
                if (t < total) {
                    const CropPos p = crop_pos(a, t, groups_x);   // (p.nv == 4)
                    float n[4], v[CT][4];
                    if (a.norm) load_px4(a.norm + p.src, 4, vec, n);
#pragma unroll
                    for (int c = 0; c < CT; ++c) load_div(a, c, p, vec, n, v[c]);
#pragma unroll
                    for (int g = 0; g < CT; ++g)
                        xchg[CT * threadIdx.x + g] = make_float4(run_elem(v, 4 * g), run_elem(v, 4 * g + 1), run_elem(v, 4 * g + 2), run_elem(v, 4 * g + 3));
                }
                __syncthreads();
                const long long live = (total - t0 < 256 ? total - t0 : 256) * CT;   // float4 this workgroup produced
                float4* o = static_cast<float4*>(a.out) + t0 * CT;
#pragma unroll
                for (int g = 0; g < CT; ++g) {
                    const int i = 256 * g + threadIdx.x;
                    if (i < live) o[i] = xchg[i];
                }
                __syncthreads();
            }
            return;
        }
    }
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const CropPos p = crop_pos(a, t, groups_x);
        float n[4];
        if (a.norm) load_px4(a.norm + p.src, p.nv, vec, n);
        if constexpr (CT == 0) {
            for (int c = 0; c < a.C; ++c) {
                float v[4];
                load_div(a, c, p, vec, n, v);
                for (int m = 0; m < p.nv; ++m) {
                    const float q[4] = {v[m], 0.f, 0.f, 0.f};
                    store_out<KIND>(a.out, (p.dst + m) * a.C + c, q, 1);
                }
            }
        } else {
            float v[CT][4];
#pragma unroll
            for (int c = 0; c < CT; ++c) load_div(a, c, p, vec, n, v[c]);
#pragma unroll
            for (int g = 0; g < CT; ++g) {
                const float b[4] = {run_elem(v, 4 * g), run_elem(v, 4 * g + 1), run_elem(v, 4 * g + 2), run_elem(v, 4 * g + 3)};
                const int left = p.nv * CT - 4 * g;
                if (left > 0) store_out<KIND>(a.out, p.dst * CT + 4 * g, b, left < 4 ? left : 4);
            }
        }
    }
}

// Both entry points, after their own argument checks: a non-empty window inside the accumulator, layout 0 | 1, kind PTB_CROP_*.
int launch_crop(const CropArgs& a, int layout, int kind, hipStream_t s) {
    const long long total = (long long)a.OD * a.OH * ((a.OW + 3) / 4);
    const long long want = (total + 255) / 256;
    const dim3 grid((unsigned)(want < 16384 ? want : 16384));
    const bool vec = !g_force_scalar && a.W % 4 == 0 && a.x0 % 4 == 0 && aligned16(a.vol) && aligned16(a.norm);
    // fp32 channel-last: exchange the lanes' runs through LDS so that the stores are lane-contiguous (C == 1 already is)
    const bool repack = !g_force_scalar && kind == PTB_CROP_F32 && a.C > 1 && a.OW % 4 == 0 && aligned16(a.out);
    with_crop_kind(kind, [&](auto k) {
        constexpr bool argmax = k() == PTB_CROP_ARGMAX_U8 || k() == PTB_CROP_ARGMAX_I64;
        if (argmax || layout == 0 || a.C == 1) {
            hipLaunchKernelGGL(crop_planar_kernel<k()>, grid, dim3(256), 0, s, a, vec);
        } else if constexpr (!argmax) {
            with_value<2, 3, 4, 0>(a.C, [&](auto c) {   // 0: C at run time
                hipLaunchKernelGGL((crop_last_kernel<k(), c()>), grid, dim3(256), 0, s, a, vec, repack); });
        }
    });
    return check_launch();
}

}  // namespace ptb

extern "C" int ptb_merge_crop(const float* image, const float* norm, int C, int H, int W, int top, int left, int OH, int OW,
                              int layout, int kind, void* out, ptb_stream_t stream) {
    if (!image || !out || C < 1 || H < 1 || W < 1 || OH < 0 || OW < 0) return PTB_EINVAL;
    if (top < 0 || left < 0 || (long long)top + OH > H || (long long)left + OW > W) return PTB_EBOUNDS;
    if (layout < 0 || layout > 1 || kind < PTB_CROP_F32 || kind > PTB_CROP_ARGMAX_I64) return PTB_EINVAL;
    if (kind == PTB_CROP_ARGMAX_U8 && C > 256) return PTB_EUNSUPPORTED;
    if (OH == 0 || OW == 0) return PTB_OK;
    return ptb::launch_crop({image, norm, out, C, 1, H, W, 0, top, left, 1, OH, OW}, layout, kind, (hipStream_t)stream);
}

extern "C" int ptb_volume_merge_crop(const float* volume, const float* norm, int C, int D, int H, int W, int z0, int y0, int x0, int OD,
                                     int OH, int OW, int layout, int kind, void* out, ptb_stream_t stream) {
    if (!volume || !norm || !out || C < 1 || D < 1 || H < 1 || W < 1 || OD < 0 || OH < 0 || OW < 0) return PTB_EINVAL;
    if (layout < 0 || layout > 1 || kind < PTB_CROP_F32 || kind > PTB_CROP_BF16) return PTB_EINVAL;
    if (z0 < 0 || y0 < 0 || x0 < 0 || (long long)z0 + OD > D || (long long)y0 + OH > H || (long long)x0 + OW > W) return PTB_EBOUNDS;
    if (kind == PTB_CROP_ARGMAX_U8 && C > 256) return PTB_EUNSUPPORTED;
    if (OD == 0 || OH == 0 || OW == 0) return PTB_OK;
    return ptb::launch_crop({volume, norm, out, C, D, H, W, z0, y0, x0, OD, OH, OW}, layout, kind, (hipStream_t)stream);
}
