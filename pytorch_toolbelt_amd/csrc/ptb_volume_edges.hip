// ptb_volume_edges.hip -- the 3-D tiled-inference loop on the device, up to the merge (the 3-D counterpart of ptb_edges.hip):
//
//   * ptb_volume_split: VolumeSlicer.split (inference/tiles_3d.py; np.pad + a copy per tile) + channels first + .float()
//     [+ per-channel affine] [+ .to(half)] from a device-resident [D, H, W(, C)] volume (uint8 / int16 / uint16 / fp16 / bf16 /
//     fp32) straight into the model batch [n, C, d, h, w].  No padded volume, no per-tile copies, no fp32 upload.
//   * ptb_volume_accumulate: VolumeMerger.integrate_batch, tile after tile into the [C, D, H, W] accumulator.
//
// The merge + crop of the accumulator is ptb_merge_crop.hip (shared with the 2-D loop).  Both kernels here are HBM-bound
// streaming kernels.  The split kernel is write-bound (4 / sizeof(in) fp32 output bytes per input byte):
// a workgroup owns a chunk of consecutive rows (z, y) of one tile, gathers it -- all channels of contiguous input row runs,
// pad voxels included -- into channel planes in LDS, then writes each channel's rows with 16-byte stores per lane (for
// full-width chunks a channel's rows are one contiguous run of the output).  ptb_volume_split_mirror (the augment end of the mirror
// TTA of ptb_volume_tta.hip) stages the same chunk (split_stage) in volume_split_views_kernel and writes it once per view: a D- or
// H-flip changes the destination row, a W-flip mirrors the column chunk and writes each lane's LDS run reversed.  The views are a
// workgroup-uniform kernel argument, not a template parameter.  The plain split keeps its own kernel: one identity view through the
// views kernel measured 0.7-1.5 % slower than the kernel below, with the same inner store loop.
#include "ptb_dispatch.h"
#include "ptb_view_device.h"

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
    // mirror views (volume_split_views_kernel; appended, so the plain split's fields keep their kernel-argument offsets)
    int nb;            // tiles of the whole call: view v of call tile b is output row v * nb + b
    int nviews, masks; // 3 bits per view (W, H, D flip); {identity} for ptb_volume_split
};

// Chunk geometry of a workgroup and the staging of its chunk: the row table, then the gather into per-channel LDS planes.
struct SplitChunk {
    int lb;              // tile within this launch group
    int plane;           // rows per tile (d * h)
    int row0, rows;      // first row (flattened z * h + y) and rows of the chunk
    int x0, cols;        // first column and columns of the chunk
};

template <int IN>
__device__ __forceinline__ SplitChunk split_stage(const VolSplitArgs& a, float* st, long long* rowoff, int tid) {
    SplitChunk k;
    int bid = blockIdx.x;
    const int cx = bid % a.ncx;
    bid /= a.ncx;
    const int cr = bid % a.ncr;
    k.lb = bid / a.ncr;
    k.plane = a.d * a.h;
    k.row0 = cr * a.R; k.rows = min(a.R, k.plane - k.row0);
    k.x0 = cx * a.XW; k.cols = min(a.XW, a.w - k.x0);
    const int lb = k.lb, row0 = k.row0, rows = k.rows, x0 = k.x0, cols = k.cols;
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
    return k;
}

template <int IN, int OUT, bool VEC>
__global__ __launch_bounds__(256) void volume_split_kernel(const VolSplitArgs a) {
    __shared__ __attribute__((aligned(16))) float st[VSPLIT_LDS];
    __shared__ long long rowoff[VSPLIT_ROWS];  // voxel index of the row's x = 0, or -1: the row lies outside the volume
    const int tid = threadIdx.x;
    const SplitChunk k = split_stage<IN>(a, st, rowoff, tid);
    const int lb = k.lb, plane = k.plane, row0 = k.row0, rows = k.rows, x0 = k.x0, cols = k.cols;
    const int C = a.C;

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

// ptb_volume_split_mirror: the chunk staged as above, then written once per view.  View k of group tile lb is output row
// k * nb + b0 + lb; a flipped view changes the destination row (d-1-z | z, h-1-y | y) and mirrors the column run (w-NV-x .. w-1-x,
// reversed in registers).
template <int IN, int OUT, bool VEC>
__global__ __launch_bounds__(256) void volume_split_views_kernel(const VolSplitArgs a) {
    __shared__ __attribute__((aligned(16))) float st[VSPLIT_LDS];
    __shared__ long long rowoff[VSPLIT_ROWS];
    const int tid = threadIdx.x;
    const SplitChunk k = split_stage<IN>(a, st, rowoff, tid);
    const int lb = k.lb, plane = k.plane, row0 = k.row0, rows = k.rows, x0 = k.x0, cols = k.cols;
    const int C = a.C;
    constexpr int NV = VEC ? (OUT == PTB_F32 ? 4 : 8) : 1;
    const int q = cols / NV;
    const int units = rows * q;
    const int dr = 256 / q, dx = 256 - dr * q;
    const int r_init = tid / q, x_init = tid - r_init * q;
    for (int view = 0; view < a.nviews; ++view) {
        const int mk = (a.masks >> (3 * view)) & 7;
        const long long tile_base = ((long long)view * a.nb + a.b0 + lb) * C;
        for (int c = 0; c < C; ++c) {
            const float sc = a.scale[c], bi = a.bias[c];
            int r = r_init, xq = x_init;
            for (int u = tid; u < units; u += 256) {
                const float* s = st + c * a.P + r * a.XW + xq * NV;
                const int rr = row0 + r, z = rr / a.h, y = rr - z * a.h;
                const int oz = (mk & 4) ? a.d - 1 - z : z, oy = (mk & 2) ? a.h - 1 - y : y;
                const int ox = (mk & 1) ? a.w - NV - (x0 + xq * NV) : x0 + xq * NV;
                const long long o = ((tile_base + c) * plane + (long long)oz * a.h + oy) * a.w + ox;
                float v[NV];
                if constexpr (VEC) {
#pragma unroll
                    for (int m = 0; m < NV; m += 4) {
                        const float4 t = *reinterpret_cast<const float4*>(s + m);
                        v[m] = t.x; v[m + 1] = t.y; v[m + 2] = t.z; v[m + 3] = t.w;
                    }
                    if (mk & 1) {
#pragma unroll
                        for (int m = 0; m < NV / 2; ++m) { const float t = v[m]; v[m] = v[NV - 1 - m]; v[NV - 1 - m] = t; }
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
}

static int launch_split(int in_dtype, int out_dtype, VolSplitArgs& g, const int64_t* zs, const int64_t* ys, const int64_t* xs, int B, bool vec,
                        hipStream_t s) {
    g.nb = B;
    const bool plain = g.nviews == 1 && g.masks == 0;  // ptb_volume_split: its own kernel, the views kernel otherwise
    for (int b0 = 0; b0 < B; b0 += VSPLIT_GROUP) {
        const int n = B - b0 < VSPLIT_GROUP ? B - b0 : VSPLIT_GROUP;
        g.b0 = b0;
        for (int t = 0; t < n; ++t) { g.tz[t] = (int)zs[b0 + t]; g.ty[t] = (int)ys[b0 + t]; g.tx[t] = (int)xs[b0 + t]; }
        const long long blocks = (long long)n * g.ncr * g.ncx;
        if (blocks > 0x7fffffffLL) return PTB_EUNSUPPORTED;
        with_value<PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16, PTB_U16>(in_dtype, [&](auto in) {
            with_value<PTB_F32, PTB_F16, PTB_BF16>(out_dtype, [&](auto out) { with_bool(vec, [&](auto v) {
                if (plain) hipLaunchKernelGGL((volume_split_kernel<in(), out(), v()>), dim3((unsigned)blocks), dim3(256), 0, s, g);
                else hipLaunchKernelGGL((volume_split_views_kernel<in(), out(), v()>), dim3((unsigned)blocks), dim3(256), 0, s, g);
            }); }); });
        if (int rc = check_launch()) return rc;
    }
    return PTB_OK;
}

// ------------------------------------------------------------------------------------------------ accumulate
// VolumeMerger.integrate_batch (reference inference/tiles_3d.py:195-208): volume[:, z:z+d, y:y+h, x:x+w] += tile * weight,
// norm_mask[...] += weight, tile after tile.  One launch per tile: a tile never overlaps itself, so every launch owns
// its accumulator region exclusively (race-free without atomics) and the stream order reproduces the reference's
// sequential fp32 order bit for bit.  A 3-D tile is megabytes, so a launch per tile is not launch-bound.
struct VolArgs {
    float* volume;        // [C, D, H, W]
    float* norm;          // [D, H, W]
    const float* weight;  // [d, h, w]
    const float* tile;    // [C, d, h, w]
    int C, d, h, w, D, H, W;
    int z0, y0, x0;
};

template <bool VEC>
__global__ __launch_bounds__(256) void volume_accumulate_kernel(const VolArgs a) {
    constexpr int PIX = VEC ? 4 : 1;
    const int wq = (a.w + PIX - 1) / PIX;
    const long long per_chan = (long long)a.d * a.h * wq;
    const long long total = per_chan * a.C;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long tplane = (long long)a.d * a.h * a.w, vplane = (long long)a.D * a.H * a.W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i / per_chan);
        long long r = i - (long long)c * per_chan;
        const int q = (int)(r % wq);
        r /= wq;
        const int y = (int)(r % a.h), z = (int)(r / a.h);
        const long long toff = ((long long)z * a.h + y) * a.w + (long long)q * PIX;
        const long long voff = ((long long)(a.z0 + z) * a.H + (a.y0 + y)) * a.W + a.x0 + (long long)q * PIX;
        if (VEC) {
            const float4 t = *reinterpret_cast<const float4*>(a.tile + c * tplane + toff);
            const float4 w4 = *reinterpret_cast<const float4*>(a.weight + toff);
            float4* vp = reinterpret_cast<float4*>(a.volume + c * vplane + voff);
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
            a.volume[c * vplane + voff] = __fadd_rn(a.volume[c * vplane + voff], __fmul_rn(a.tile[c * tplane + toff], wv));
            if (c == 0) a.norm[voff] = __fadd_rn(a.norm[voff], wv);
        }
    }
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_volume_split_mirror(const void* volume, int in_dtype, int D, int H, int W, int C, const int64_t* zs,
                                       const int64_t* ys, const int64_t* xs, int B, int d, int h, int w, const float* scale,
                                       const float* bias, float pad_value, int nviews, const int* masks, int out_dtype, void* out,
                                       ptb_stream_t stream) {
    if (!volume || !out || !zs || !ys || !xs || D < 1 || H < 1 || W < 1 || C < 1 || B < 0 || d < 1 || h < 1 || w < 1) return PTB_EINVAL;
    if (in_dtype < PTB_F32 || in_dtype > PTB_U16 || out_dtype < PTB_F32 || out_dtype > PTB_BF16) return PTB_EINVAL;
    if ((scale == nullptr) != (bias == nullptr)) return PTB_EINVAL;
    if (C > MAX_VSPLIT_C) return PTB_EUNSUPPORTED;
    if (nviews < 1 || nviews > MAX_VIEWS || !masks) return PTB_EINVAL;
    int packed = 0;
    for (int k = 0; k < nviews; ++k) {
        if (masks[k] < 0 || masks[k] > 7) return PTB_EINVAL;
        packed |= masks[k] << (3 * k);
    }
    if ((long long)d * h > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    for (int b = 0; b < B; ++b) {  // a tile may overhang any face but must be addressable with 32-bit coordinates
        const int64_t o[3] = {zs[b], ys[b], xs[b]};
        for (int k = 0; k < 3; ++k)
            if (o[k] < -(1 << 30) || o[k] > (1 << 30)) return PTB_EBOUNDS;
    }
    if (B == 0) return PTB_OK;
    VolSplitArgs g{};
    g.nviews = nviews; g.masks = packed;
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
    return launch_split(in_dtype, out_dtype, g, zs, ys, xs, B, vec, s);
}

// ptb_volume_split keeps its own first checks, in their order, and is the split with the single identity view
extern "C" int ptb_volume_split(const void* volume, int in_dtype, int D, int H, int W, int C, const int64_t* zs, const int64_t* ys,
                                const int64_t* xs, int B, int d, int h, int w, const float* scale, const float* bias, float pad_value,
                                int out_dtype, void* out, ptb_stream_t stream) {
    if (!volume || !out || !zs || !ys || !xs || D < 1 || H < 1 || W < 1 || C < 1 || B < 0 || d < 1 || h < 1 || w < 1) return PTB_EINVAL;
    if (in_dtype < PTB_F32 || in_dtype > PTB_U16 || out_dtype < PTB_F32 || out_dtype > PTB_BF16) return PTB_EINVAL;
    if ((scale == nullptr) != (bias == nullptr)) return PTB_EINVAL;
    if (C > MAX_VSPLIT_C) return PTB_EUNSUPPORTED;
    const int ident = 0;
    return ptb_volume_split_mirror(volume, in_dtype, D, H, W, C, zs, ys, xs, B, d, h, w, scale, bias, pad_value, 1, &ident, out_dtype,
                                   out, stream);
}

extern "C" int ptb_volume_accumulate(float* volume, float* norm, const float* weight, const float* tiles, const int64_t* zs,
                                     const int64_t* ys, const int64_t* xs, int B, int C, int d, int h, int w, int D, int H, int W,
                                     ptb_stream_t stream) {
    if (!volume || !norm || !weight || !tiles || !zs || !ys || !xs) return PTB_EINVAL;
    if (B < 0 || C < 1 || d < 1 || h < 1 || w < 1 || D < 1 || H < 1 || W < 1) return PTB_EINVAL;
    for (int b = 0; b < B; ++b)
        if (zs[b] < 0 || ys[b] < 0 || xs[b] < 0 || zs[b] + d > D || ys[b] + h > H || xs[b] + w > W) return PTB_EBOUNDS;
    VolArgs a{volume, norm, weight, nullptr, C, d, h, w, D, H, W, 0, 0, 0};
    const long long tile_elems = (long long)C * d * h * w;
    const bool base_vec = !g_force_scalar && w % 4 == 0 && W % 4 == 0 && aligned16(volume) && aligned16(norm) && aligned16(weight) &&
                          aligned16(tiles) && tile_elems % 4 == 0;
    for (int b = 0; b < B; ++b) {
        a.tile = tiles + (long long)b * tile_elems;
        a.z0 = (int)zs[b]; a.y0 = (int)ys[b]; a.x0 = (int)xs[b];
        const bool vec = base_vec && a.x0 % 4 == 0;
        const long long items = (long long)C * d * h * (vec ? w / 4 : w);
        const long long want = (items + 255) / 256;
        const dim3 grid((unsigned)(want < 16384 ? want : 16384)), block(256);
        with_bool(vec, [&](auto v) { hipLaunchKernelGGL(ptb::volume_accumulate_kernel<v()>, grid, block, 0, (hipStream_t)stream, a); });
        if (int rc = ptb::check_launch()) return rc;
    }
    return PTB_OK;
}
