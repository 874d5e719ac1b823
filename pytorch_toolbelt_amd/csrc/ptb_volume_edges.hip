// ptb_volume_edges.hip -- the two ends of the 3-D tiled-inference loop, on the device (the 3-D counterpart of ptb_edges.hip):
//
//   * ptb_volume_split: VolumeSlicer.split (inference/tiles_3d.py; np.pad + a copy per tile) + channels first + .float()
//     [+ per-channel affine] [+ .to(half)] from a device-resident [D, H, W(, C)] volume (uint8 / int16 / uint16 / fp16 / bf16 /
//     fp32) straight into the model batch [n, C, d, h, w].  No padded volume, no per-tile copies, no fp32 upload.
//   * ptb_volume_merge_crop: VolumeMerger.merge (volume / norm_mask, ptb_merge_div) + crop to VolumeSlicer.orignal_image_roi
//     [+ channels last] [+ cast | argmax over channels] in one pass that reads and writes only the cropped window.
//
// Both are HBM-bound streaming kernels.  The split kernel is write-bound (4 / sizeof(in) fp32 output bytes per input byte):
// a workgroup owns a chunk of consecutive rows (z, y) of one tile, gathers it -- all channels of contiguous input row runs,
// pad voxels included -- into channel planes in LDS, then writes each channel's rows with 16-byte stores per lane (for
// full-width chunks a channel's rows are one contiguous run of the output).
#include "ptb_edges_device.h"

namespace ptb {

constexpr int MAX_VSPLIT_C = 16;
constexpr int VSPLIT_GROUP = 64;      // tiles per launch (kernarg budget: 3 x 64 origins)
constexpr int VSPLIT_LDS = 4096;      // floats of channel planes staged per workgroup (16 KiB)
constexpr int VSPLIT_ROWS = 256;      // at most one row per thread: the row table is filled in one step

struct VolSplitArgs {
    const void* vol;   // [D, H, W, C] contiguous
    void* out;         // [B, C, d, h, w]
    int D, H, W, C;
    int d, h, w;
    int XW, R, P;      // chunk columns, chunk rows (flattened z * h + y), LDS plane stride (floats)
    int ncx, ncr;      // column chunks and row chunks per tile
    int b0;            // batch index of the first tile of this launch group
    float pad;         // border value, already cast to the volume's dtype
    int affine;        // 1: out = in * scale[c] + bias[c] (two roundings, like torch)
    float scale[MAX_VSPLIT_C], bias[MAX_VSPLIT_C];
    int tz[VSPLIT_GROUP], ty[VSPLIT_GROUP], tx[VSPLIT_GROUP];  // tile origins in volume coordinates; may overhang any face
};

// element i of the volume as fp32 (exact for every supported dtype); IN = PTB_F32 .. PTB_U16
template <int IN>
__device__ __forceinline__ float widen(const void* p, long long i) {
    if constexpr (IN == PTB_F32) return static_cast<const float*>(p)[i];
    else if constexpr (IN == PTB_F16) return (float)static_cast<const _Float16*>(p)[i];
    else if constexpr (IN == PTB_BF16) return __uint_as_float((unsigned)static_cast<const unsigned short*>(p)[i] << 16);
    else if constexpr (IN == PTB_U8) return (float)static_cast<const uint8_t*>(p)[i];
    else if constexpr (IN == PTB_I16) return (float)static_cast<const int16_t*>(p)[i];
    else return (float)static_cast<const uint16_t*>(p)[i];
}

template <int IN, int OUT, bool VEC>
__global__ __launch_bounds__(256) void volume_split_kernel(const VolSplitArgs a) {
    __shared__ __attribute__((aligned(16))) float st[VSPLIT_LDS];
    __shared__ long long rowoff[VSPLIT_ROWS];  // voxel index of the row's x = 0, or -1: the row lies outside the volume
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int cx = bid % a.ncx;
    bid /= a.ncx;
    const int cr = bid % a.ncr;
    const int lb = bid / a.ncr;  // tile within this launch group
    const int plane = a.d * a.h;
    const int row0 = cr * a.R, rows = min(a.R, plane - row0);
    const int x0 = cx * a.XW, cols = min(a.XW, a.w - x0);
    const int C = a.C;
    if (tid < rows) {
        const int rr = row0 + tid, z = rr / a.h, y = rr - z * a.h;
        const int gz = a.tz[lb] + z, gy = a.ty[lb] + y;
        rowoff[tid] = (gz >= 0 && gz < a.D && gy >= 0 && gy < a.H) ? ((long long)gz * a.H + gy) * a.W : -1;
    }
    __syncthreads();

    // gather: element e of the chunk is (row r, column x, channel c) with e = (r * cols + x) * C + c -- consecutive lanes read
    // consecutive input elements of a row run and write them to their channel plane (the de-interleave)
    {
        const int run = cols * C;
        const int total = rows * run;
        const int dr = 256 / run, dk = 256 - dr * run, dkx = dk / C, dkc = dk - dkx * C;
        int r = tid / run;
        const int k = tid - r * run;
        int x = k / C, c = k - (k / C) * C;
        const int gx0 = a.tx[lb] + x0;
        for (int e = tid; e < total; e += 256) {
            const long long ro = rowoff[r];
            const int gx = gx0 + x;
            float f = a.pad;
            if (ro >= 0 && gx >= 0 && gx < a.W) f = widen<IN>(a.vol, (ro + gx) * C + c);
            st[c * a.P + r * a.XW + x] = f;
            c += dkc; x += dkx; r += dr;
            if (c >= C) { c -= C; ++x; }
            if (x >= cols) { x -= cols; ++r; }
        }
    }
    __syncthreads();

    // store: channel by channel (uniform, so scale[c] / bias[c] stay scalar loads), NV consecutive outputs per lane
    constexpr int NV = VEC ? (OUT == PTB_F32 ? 4 : 8) : 1;
    const int q = cols / NV;  // (VEC: cols is a multiple of NV)
    const int units = rows * q;
    const int dr = 256 / q, dx = 256 - dr * q;
    const int r_init = tid / q, x_init = tid - r_init * q;
    const long long tile_base = (long long)(a.b0 + lb) * C;
    for (int c = 0; c < C; ++c) {
        const float sc = a.scale[c], bi = a.bias[c];
        const long long cbase = ((tile_base + c) * plane + row0) * a.w + x0;
        int r = r_init, xq = x_init;
        for (int u = tid; u < units; u += 256) {
            const float* s = st + c * a.P + r * a.XW + xq * NV;
            const long long o = cbase + (long long)r * a.w + xq * NV;
            float v[NV];
            if constexpr (VEC) {
#pragma unroll
                for (int m = 0; m < NV; m += 4) {
                    const float4 t = *reinterpret_cast<const float4*>(s + m);
                    v[m] = t.x; v[m + 1] = t.y; v[m + 2] = t.z; v[m + 3] = t.w;
                }
            } else {
                v[0] = s[0];
            }
            if (a.affine) {
#pragma unroll
                for (int m = 0; m < NV; ++m) v[m] = __fadd_rn(__fmul_rn(v[m], sc), bi);
            }
            if constexpr (OUT == PTB_F32) {
                if constexpr (VEC) out_store4(static_cast<float*>(a.out) + o, make_float4(v[0], v[1], v[2], v[3]));
                else static_cast<float*>(a.out)[o] = v[0];
            } else {
                if constexpr (VEC) {
                    unsigned w4[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) w4[m] = (unsigned)half_bits<OUT>(v[2 * m]) | ((unsigned)half_bits<OUT>(v[2 * m + 1]) << 16);
                    out_store4(reinterpret_cast<float*>(static_cast<unsigned short*>(a.out) + o),
                               make_float4(__uint_as_float(w4[0]), __uint_as_float(w4[1]), __uint_as_float(w4[2]), __uint_as_float(w4[3])));
                } else {
                    static_cast<unsigned short*>(a.out)[o] = half_bits<OUT>(v[0]);
                }
            }
            xq += dx; r += dr;
            if (xq >= q) { xq -= q; ++r; }
        }
    }
}

// ------------------------------------------------------------------------------------------------ merge + crop
enum { VCROP_F32 = PTB_CROP_F32, VCROP_U8 = PTB_CROP_U8, VCROP_ARGMAX_U8 = PTB_CROP_ARGMAX_U8, VCROP_ARGMAX_I64 = PTB_CROP_ARGMAX_I64,
       VCROP_F16 = PTB_CROP_F16, VCROP_BF16 = PTB_CROP_BF16 };

struct VolCropArgs {
    const float* vol;   // [C, D, H, W] accumulator
    const float* norm;  // [D, H, W]
    void* out;
    int C, D, H, W;
    int z0, y0, x0, OD, OH, OW;
};

// nv (<= 4) consecutive output elements starting at element `o`, converted to KIND; one 16 / 8 / 4 B store when aligned
template <int KIND>
__device__ __forceinline__ void store_out(void* out, long long o, const float* v, int nv) {
    if constexpr (KIND == VCROP_F32) {
        store_f32x4(static_cast<float*>(out) + o, v, nv);
    } else if constexpr (KIND == VCROP_U8) {
        uint8_t b[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) b[m] = cast_u8(v[m]);
        store_u8x4(static_cast<uint8_t*>(out) + o, b, nv);
    } else {
        constexpr int OUT = KIND == VCROP_F16 ? PTB_F16 : PTB_BF16;
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

// Output voxel group t (4 consecutive x of one output row) -> its source offset, output voxel offset and width
struct CropPos { long long src, dst; int nv; };
__device__ __forceinline__ CropPos crop_pos(const VolCropArgs& a, long long t, int groups_x) {
    const long long row = t / groups_x;
    const int x = (int)(t - row * groups_x) * 4;
    const int z = (int)(row / a.OH), y = (int)(row - (long long)z * a.OH);
    CropPos p;
    p.src = ((long long)(a.z0 + z) * a.H + a.y0 + y) * a.W + a.x0 + x;
    p.dst = row * a.OW + x;
    p.nv = min(4, a.OW - x);
    return p;
}

// Channel-planar outputs ([C, OD, OH, OW]) and argmax: one pass over the channels with running state, any C.
template <int KIND>
__global__ __launch_bounds__(256) void volume_crop_planar_kernel(const VolCropArgs a, bool vec) {
    const int groups_x = (a.OW + 3) / 4;
    const long long total = (long long)a.OD * a.OH * groups_x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long iplane = (long long)a.D * a.H * a.W, oplane = (long long)a.OD * a.OH * a.OW;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const CropPos p = crop_pos(a, t, groups_x);
        float n[4], v[4];
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int arg[4] = {0, 0, 0, 0};
        load_px4(a.norm + p.src, p.nv, vec, n);
        for (int c = 0; c < a.C; ++c) {
            load_px4(a.vol + c * iplane + p.src, p.nv, vec, v);
#pragma unroll
            for (int m = 0; m < 4; ++m) v[m] = __fdiv_rn(v[m], n[m]);  // ptb_merge_div: no eps clamp
            if constexpr (KIND == VCROP_ARGMAX_U8 || KIND == VCROP_ARGMAX_I64) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {  // first maximum wins; NaN counts as the maximum (torch argmax)
                    const bool take = c == 0 ? true : (v[m] > best[m] || (v[m] != v[m] && best[m] == best[m]));
                    best[m] = take ? v[m] : best[m];
                    arg[m] = take ? c : arg[m];
                }
            } else {
                store_out<KIND>(a.out, c * oplane + p.dst, v, p.nv);
            }
        }
        if constexpr (KIND == VCROP_ARGMAX_U8) {
            uint8_t b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) b[m] = (uint8_t)arg[m];
            store_u8x4(static_cast<uint8_t*>(a.out) + p.dst, b, p.nv);
        } else if constexpr (KIND == VCROP_ARGMAX_I64) {
            long long* o = static_cast<long long*>(a.out) + p.dst;
            for (int m = 0; m < p.nv; ++m) o[m] = arg[m];
        }
    }
}

// Channel-last outputs ([OD, OH, OW, C]).  CT in 2..4: the CT channels of 4 voxels held in registers, so the thread's 4 * CT
// contiguous output elements leave as CT full-width stores.  CT == 0: any C, element by element (not a tuned path).
template <int KIND, int CT>
__global__ __launch_bounds__(256) void volume_crop_dhwc_kernel(const VolCropArgs a, bool vec) {
    const int groups_x = (a.OW + 3) / 4;
    const long long total = (long long)a.OD * a.OH * groups_x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long iplane = (long long)a.D * a.H * a.W;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const CropPos p = crop_pos(a, t, groups_x);
        float n[4];
        load_px4(a.norm + p.src, p.nv, vec, n);
        if constexpr (CT == 0) {
            for (int c = 0; c < a.C; ++c) {
                float v[4];
                load_px4(a.vol + c * iplane + p.src, p.nv, vec, v);
                for (int m = 0; m < p.nv; ++m) {
                    const float q[4] = {__fdiv_rn(v[m], n[m]), 0.f, 0.f, 0.f};
                    store_out<KIND>(a.out, (p.dst + m) * a.C + c, q, 1);
                }
            }
        } else {
            float v[CT][4];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                load_px4(a.vol + c * iplane + p.src, p.nv, vec, v[c]);
#pragma unroll
                for (int m = 0; m < 4; ++m) v[c][m] = __fdiv_rn(v[c][m], n[m]);
            }
            // element e = m * CT + c of the thread's contiguous run; group g = elements 4g .. 4g+3
#pragma unroll
            for (int g = 0; g < CT; ++g) {
                float b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = v[(4 * g + j) % CT][(4 * g + j) / CT];
                const int left = p.nv * CT - 4 * g;
                if (left > 0) store_out<KIND>(a.out, p.dst * CT + 4 * g, b, left < 4 ? left : 4);
            }
        }
    }
}

template <int IN, int OUT>
int launch_split(VolSplitArgs& g, const int64_t* zs, const int64_t* ys, const int64_t* xs, int B, bool vec, hipStream_t s) {
    for (int b0 = 0; b0 < B; b0 += VSPLIT_GROUP) {
        const int n = B - b0 < VSPLIT_GROUP ? B - b0 : VSPLIT_GROUP;
        g.b0 = b0;
        for (int t = 0; t < n; ++t) { g.tz[t] = (int)zs[b0 + t]; g.ty[t] = (int)ys[b0 + t]; g.tx[t] = (int)xs[b0 + t]; }
        const long long blocks = (long long)n * g.ncr * g.ncx;
        if (blocks > 0x7fffffffLL) return PTB_EUNSUPPORTED;
        if (vec) hipLaunchKernelGGL((volume_split_kernel<IN, OUT, true>), dim3((unsigned)blocks), dim3(256), 0, s, g);
        else hipLaunchKernelGGL((volume_split_kernel<IN, OUT, false>), dim3((unsigned)blocks), dim3(256), 0, s, g);
        if (int rc = check_launch()) return rc;
    }
    return PTB_OK;
}

template <int IN>
int launch_split_in(int out_dtype, VolSplitArgs& g, const int64_t* zs, const int64_t* ys, const int64_t* xs, int B, bool vec, hipStream_t s) {
    if (out_dtype == PTB_F32) return launch_split<IN, PTB_F32>(g, zs, ys, xs, B, vec, s);
    if (out_dtype == PTB_F16) return launch_split<IN, PTB_F16>(g, zs, ys, xs, B, vec, s);
    return launch_split<IN, PTB_BF16>(g, zs, ys, xs, B, vec, s);
}

template <int KIND>
void launch_crop(const VolCropArgs& a, int layout, bool vec, dim3 grid, hipStream_t s) {
    if constexpr (KIND == VCROP_ARGMAX_U8 || KIND == VCROP_ARGMAX_I64) {
        hipLaunchKernelGGL(volume_crop_planar_kernel<KIND>, grid, dim3(256), 0, s, a, vec);
    } else {
        if (layout == 0 || a.C == 1) hipLaunchKernelGGL(volume_crop_planar_kernel<KIND>, grid, dim3(256), 0, s, a, vec);
        else if (a.C == 2) hipLaunchKernelGGL((volume_crop_dhwc_kernel<KIND, 2>), grid, dim3(256), 0, s, a, vec);
        else if (a.C == 3) hipLaunchKernelGGL((volume_crop_dhwc_kernel<KIND, 3>), grid, dim3(256), 0, s, a, vec);
        else if (a.C == 4) hipLaunchKernelGGL((volume_crop_dhwc_kernel<KIND, 4>), grid, dim3(256), 0, s, a, vec);
        else hipLaunchKernelGGL((volume_crop_dhwc_kernel<KIND, 0>), grid, dim3(256), 0, s, a, vec);
    }
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_volume_split(const void* volume, int in_dtype, int D, int H, int W, int C, const int64_t* zs, const int64_t* ys,
                                const int64_t* xs, int B, int d, int h, int w, const float* scale, const float* bias, float pad_value,
                                int out_dtype, void* out, ptb_stream_t stream) {
    if (!volume || !out || !zs || !ys || !xs || D < 1 || H < 1 || W < 1 || C < 1 || B < 0 || d < 1 || h < 1 || w < 1) return PTB_EINVAL;
    if (in_dtype < PTB_F32 || in_dtype > PTB_U16 || out_dtype < PTB_F32 || out_dtype > PTB_BF16) return PTB_EINVAL;
    if ((scale == nullptr) != (bias == nullptr)) return PTB_EINVAL;
    if (C > MAX_VSPLIT_C) return PTB_EUNSUPPORTED;
    if ((long long)d * h > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    for (int b = 0; b < B; ++b) {  // a tile may overhang any face but must be addressable with 32-bit coordinates
        const int64_t o[3] = {zs[b], ys[b], xs[b]};
        for (int k = 0; k < 3; ++k)
            if (o[k] < -(1 << 30) || o[k] > (1 << 30)) return PTB_EBOUNDS;
    }
    if (B == 0) return PTB_OK;
    VolSplitArgs g{};
    g.vol = volume; g.out = out;
    g.D = D; g.H = H; g.W = W; g.C = C;
    g.d = d; g.h = h; g.w = w;
    g.pad = pad_value;
    g.affine = scale ? 1 : 0;
    for (int c = 0; c < C; ++c) { g.scale[c] = scale ? scale[c] : 1.0f; g.bias[c] = bias ? bias[c] : 0.0f; }
    // chunk geometry: C planes of P = R * XW + 4 floats fit the LDS budget (+4: channel planes start on different banks)
    const int nv = out_dtype == PTB_F32 ? 4 : 8;
    const bool vec = !g_force_scalar && w % nv == 0 && aligned16(out);
    const int per = VSPLIT_LDS / C - 4;
    g.XW = w <= per ? w : (vec ? per / nv * nv : per);
    const long long rows = (long long)d * h;
    long long R = per / g.XW;
    R = R < rows ? R : rows;
    g.R = (int)(R < VSPLIT_ROWS ? R : VSPLIT_ROWS);
    g.P = g.R * g.XW + 4;
    g.ncx = (w + g.XW - 1) / g.XW;
    g.ncr = (int)((rows + g.R - 1) / g.R);
    hipStream_t s = (hipStream_t)stream;
    switch (in_dtype) {
        case PTB_F32: return launch_split_in<PTB_F32>(out_dtype, g, zs, ys, xs, B, vec, s);
        case PTB_F16: return launch_split_in<PTB_F16>(out_dtype, g, zs, ys, xs, B, vec, s);
        case PTB_BF16: return launch_split_in<PTB_BF16>(out_dtype, g, zs, ys, xs, B, vec, s);
        case PTB_U8: return launch_split_in<PTB_U8>(out_dtype, g, zs, ys, xs, B, vec, s);
        case PTB_I16: return launch_split_in<PTB_I16>(out_dtype, g, zs, ys, xs, B, vec, s);
        default: return launch_split_in<PTB_U16>(out_dtype, g, zs, ys, xs, B, vec, s);
    }
}

extern "C" int ptb_volume_merge_crop(const float* volume, const float* norm, int C, int D, int H, int W, int z0, int y0, int x0, int OD,
                                     int OH, int OW, int layout, int kind, void* out, ptb_stream_t stream) {
    if (!volume || !norm || !out || C < 1 || D < 1 || H < 1 || W < 1 || OD < 0 || OH < 0 || OW < 0) return PTB_EINVAL;
    if (layout < 0 || layout > 1 || kind < VCROP_F32 || kind > VCROP_BF16) return PTB_EINVAL;
    if (z0 < 0 || y0 < 0 || x0 < 0 || (long long)z0 + OD > D || (long long)y0 + OH > H || (long long)x0 + OW > W) return PTB_EBOUNDS;
    if (kind == VCROP_ARGMAX_U8 && C > 256) return PTB_EUNSUPPORTED;
    if (OD == 0 || OH == 0 || OW == 0) return PTB_OK;
    const VolCropArgs a{volume, norm, out, C, D, H, W, z0, y0, x0, OD, OH, OW};
    const long long total = (long long)OD * OH * ((OW + 3) / 4);
    const long long want = (total + 255) / 256;
    const dim3 grid((unsigned)(want < 16384 ? want : 16384));
    hipStream_t s = (hipStream_t)stream;
    const bool vec = !g_force_scalar && W % 4 == 0 && x0 % 4 == 0 && aligned16(volume) && aligned16(norm);
    switch (kind) {
        case VCROP_F32: launch_crop<VCROP_F32>(a, layout, vec, grid, s); break;
        case VCROP_U8: launch_crop<VCROP_U8>(a, layout, vec, grid, s); break;
        case VCROP_ARGMAX_U8: launch_crop<VCROP_ARGMAX_U8>(a, layout, vec, grid, s); break;
        case VCROP_ARGMAX_I64: launch_crop<VCROP_ARGMAX_I64>(a, layout, vec, grid, s); break;
        case VCROP_F16: launch_crop<VCROP_F16>(a, layout, vec, grid, s); break;
        default: launch_crop<VCROP_BF16>(a, layout, vec, grid, s); break;
    }
    return check_launch();
}
