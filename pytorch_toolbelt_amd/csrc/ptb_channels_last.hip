// ptb_channels_last.hip -- the view-gather family on channels-last model outputs (PTB_SRC_CHANNELS_LAST), gfx950 / MI355X.
//
// A model in torch.channels_last returns [V*B, th, tw, C] memory: the C channels of a pixel lie next to each other.  These kernels do
// what view_plain_kernel / view_accum_kernel / band_merge_kernel / band_plan_kernel do (ptb_views.hip, ptb_bandplan.hip) and write
// what they write -- planar fp32 -- but read such a source where it lies, so the [V*B, C, th, tw] copy never exists.
//
// Work division: a view of the D4 group permutes PIXELS, and here a pixel is one contiguous run of C elements, so no transposition is
// needed at all -- not in LDS, not in registers: a lane owns one output pixel, fetches that pixel's channels from each view's mirrored /
// transposed position (one 16-byte load per view for four fp32 channels, 8 bytes for four half channels), reduces over the views in
// registers and blends.  A wave covers 4 rows x 16 pixels of the output: row-preserving views read 4 runs of 16 x C elements,
// transposing views 16 runs of 4 x C, and the other half of those lines is read by the next wave of the same workgroup.  One
// workgroup (256 threads) walks a whole chunk / work item over ALL channels, four at a time, so window and normaliser are read once
// per pixel and the host's chunk tables are consumed unchanged.  C is a run-time value; a source whose C is a multiple of 4 (and whose
// tiles are 16- / 8-byte aligned) takes the vector loads, any other C takes element loads of the same four channels.  No LDS, no
// barrier, no scratch.
//
// Per pixel and channel the arithmetic is the planar kernels': views summed in view order with __fadd_rn, red_pre / red_post /
// div_views, PTB_ROUND_SRC, then tile * window rounded and added in integration order (no contraction) -- bit-identical results.
#include "ptb_dispatch.h"
#include "ptb_view_device.h"

namespace ptb {

namespace {

constexpr int CL_THREADS = 256;   // 16 x 16 pixels per pass of a workgroup over its chunk
constexpr int CL_NC = 4;          // channels a lane handles at a time

template <int IN> struct LdOf { static constexpr int value = IN == PTB_F32 ? 0 : (IN == PTB_F16 ? 2 : 3); };   // ld4 / round_src4 selector

// channels c0 .. c0+3 of the pixel whose channel 0 is element `off` of `base`; channels >= nc stay 1 (never stored)
template <int IN, bool VEC>
__device__ __forceinline__ float4 cl_load(const float* base, long long off, int nc) {
    if constexpr (VEC) {
        return ld4<LdOf<IN>::value>(base, off);
    } else {
        float4 v = make_float4(1.f, 1.f, 1.f, 1.f);
        v.x = widen<IN>(base, off);
        if (nc > 1) v.y = widen<IN>(base, off + 1);
        if (nc > 2) v.z = widen<IN>(base, off + 2);
        if (nc > 3) v.w = widen<IN>(base, off + 3);
        return v;
    }
}

// Reduced value of channels c0 .. c0+3 of output pixel (i, j) of one tile; `off0` = element offset of view 0 of the tile in `base`.
template <int OPK, int IN, bool VEC>
__device__ __forceinline__ float4 cl_reduce_px(const float* __restrict__ base, long long off0, long long view_stride, int nv, int codes, int H, int W,
                                               int C, int i, int j, int c0, int nc, int op, float divisor) {
    float4 v[MAX_VIEWS];
#pragma unroll
    for (int k = 0; k < MAX_VIEWS; ++k) {
        v[k] = make_float4(1.f, 1.f, 1.f, 1.f);
        if (k < nv) {
            const int code = (codes >> (3 * k)) & 7;      // out[i][j] = src[rr][cc]: the mapping of scalar_reduce (ptb_views.hip)
            int rr = (code & 1) ? j : i, cc = (code & 1) ? i : j;
            const int rows = (code & 1) ? W : H, cols = (code & 1) ? H : W;
            if (code & 2) rr = rows - 1 - rr;
            if (code & 4) cc = cols - 1 - cc;
            v[k] = cl_load<IN, VEC>(base, off0 + (long long)k * view_stride + ((long long)rr * cols + cc) * C + c0, nc);
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

// acc += reduced tile value * window, channels c0 .. c0+3 (tiles.py:338: the product rounded, then added -- no FMA contraction)
template <int OPK, int IN, bool VEC>
__device__ __forceinline__ void cl_blend(const ViewArgs& a, const float* __restrict__ base, long long off0, long long view_stride, int li, int lj, int c0,
                                         int nc, float w, float4& acc) {
    const float4 val = round_src4<LdOf<IN>::value>(
        cl_reduce_px<OPK, IN, VEC>(base, off0, view_stride, a.nviews, a.codes, a.H, a.W, a.C, li, lj, c0, nc, a.op, a.divisor), a.round_src);
    acc.x = __fadd_rn(acc.x, __fmul_rn(val.x, w));
    acc.y = __fadd_rn(acc.y, __fmul_rn(val.y, w));
    acc.z = __fadd_rn(acc.z, __fmul_rn(val.z, w));
    acc.w = __fadd_rn(acc.w, __fmul_rn(val.w, w));
}

__device__ __forceinline__ float4 cl_load_planes(const float* p, long long chan_stride, int nc) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    v.x = p[0];
    if (nc > 1) v.y = p[chan_stride];
    if (nc > 2) v.z = p[2 * chan_stride];
    if (nc > 3) v.w = p[3 * chan_stride];
    return v;
}
__device__ __forceinline__ void cl_store_planes(float* p, long long chan_stride, int nc, const float4 v) {
    p[0] = v.x;
    if (nc > 1) p[chan_stride] = v.y;
    if (nc > 2) p[2 * chan_stride] = v.z;
    if (nc > 3) p[3 * chan_stride] = v.w;
}
__device__ __forceinline__ float4 cl_div(const float4 s, float n) {   // tiles.py:346
    return make_float4(__fdiv_rn(s.x, n), __fdiv_rn(s.y, n), __fdiv_rn(s.z, n), __fdiv_rn(s.w, n));
}

}  // namespace

// ------------------------------------------------------------------------------------------------ de-augment + reduce (view_plain_kernel, MODE_REDUCE)
template <int OPK, int IN, bool VEC>
__global__ __launch_bounds__(CL_THREADS) void cl_reduce_kernel(const ViewArgs a, int chrows) {
    const int cpt = a.chunks_x * a.chunks_y;
    const int chunk = blockIdx.x % cpt, t = blockIdx.x / cpt;
    const int cx0 = (chunk % a.chunks_x) * CW, cy0 = (chunk / a.chunks_x) * chrows;
    const int cw = min(CW, a.W - cx0), ch = min(chrows, a.H - cy0);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long off0 = (long long)t * a.src_tile_stride;
    for (int r = ty; r < ch; r += 16) {
        for (int x = tx; x < cw; x += 16) {
            const int i = cy0 + r, j = cx0 + x;
            float* o = a.dst + (long long)t * a.dst_tile_stride + (long long)i * a.dst_row_stride + j;
            for (int c0 = 0; c0 < a.C; c0 += CL_NC) {
                const int nc = min(CL_NC, a.C - c0);
                const float4 val = cl_reduce_px<OPK, IN, VEC>(a.src, off0, a.src_view_stride, a.nviews, a.codes, a.H, a.W, a.C, i, j, c0, nc, a.op, a.divisor);
                cl_store_planes(o + (long long)c0 * a.dst_chan_stride, a.dst_chan_stride, nc, val);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ accumulate (view_accum_kernel)
// Same cells, same chunk walk, same first-touch / final handling; blockIdx.x = chunk (all channels).
template <int OPK, int IN, bool VEC>
__global__ __launch_bounds__(CL_THREADS) void cl_accum_kernel(const ViewArgs a, const CellArgs g, int chrows) {
    const int chunk = blockIdx.x;
    int ci = 0;
    while (ci < a.ncells - 1 && chunk >= g.cells[ci].chunk_end) ++ci;
    const Cell& cell = g.cells[ci];
    const int first = ci ? g.cells[ci - 1].chunk_end : 0;
    const int ncx = (cell.w + CW - 1) / CW;
    const int lc = chunk - first;
    const int cx0 = (lc % ncx) * CW, cy0 = (lc / ncx) * chrows;
    const int cw = min(CW, cell.w - cx0), ch = min(chrows, cell.h - cy0);
    const int ax = cell.ox + cx0, ay = cell.oy + cy0;  // chunk origin in the accumulator
    const int nt = cell.ntiles, fresh = cell.fresh, fin = cell.final_;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    for (int r = ty; r < ch; r += 16) {
        for (int x = tx; x < cw; x += 16) {
            const long long pix = (long long)(ay + r) * a.dst_row_stride + ax + x;
            float wv[MAX_COVER];
#pragma unroll
            for (int e = 0; e < MAX_COVER; ++e) {
                wv[e] = 0.f;
                if (e < nt) {
                    const int gt = cell.tile[e];
                    wv[e] = a.weight[(long long)(ay + r - g.tile_y[gt]) * a.W + ax + x - g.tile_x[gt]];
                }
            }
            const float nfull = fin ? a.norm_full[pix] : 1.f;
            if (a.norm != nullptr && !fin) {   // norm == NULL: the caller keeps the (data independent) normaliser itself
                float nacc = fresh ? 0.f : a.norm[pix];
#pragma unroll
                for (int e = 0; e < MAX_COVER; ++e)
                    if (e < nt) nacc = __fadd_rn(nacc, wv[e]);
                a.norm[pix] = nacc;
            }
            for (int c0 = 0; c0 < a.C; c0 += CL_NC) {
                const int nc = min(CL_NC, a.C - c0);
                float* ip = a.dst + (long long)c0 * a.dst_chan_stride + pix;
                float4 acc = fresh ? make_float4(0.f, 0.f, 0.f, 0.f) : cl_load_planes(ip, a.dst_chan_stride, nc);
#pragma unroll
                for (int e = 0; e < MAX_COVER; ++e) {
                    if (e < nt) {
                        const int gt = cell.tile[e];
                        cl_blend<OPK, IN, VEC>(a, a.src, (long long)g.tile_id[gt] * a.src_tile_stride, a.src_view_stride, ay + r - g.tile_y[gt],
                                               ax + x - g.tile_x[gt], c0, nc, wv[e], acc);
                    }
                }
                if (fin) {
                    cl_store_planes(a.merged + (long long)c0 * a.dst_chan_stride + pix, a.dst_chan_stride, nc, cl_div(acc, nfull));
                    if (a.keep_acc) cl_store_planes(ip, a.dst_chan_stride, nc, acc);
                } else {
                    cl_store_planes(ip, a.dst_chan_stride, nc, acc);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ one band (band_merge_kernel, 32-row chunks)
template <int OPK, int IN, bool VEC>
__global__ __launch_bounds__(CL_THREADS) void cl_band_kernel(const ViewArgs a, const BandArgs g) {
    constexpr int CH = 32;
    const int chunk = blockIdx.x;
    int ci = 0;
    while (ci < a.ncells - 1 && chunk >= g.cells[ci].chunk_end) ++ci;
    const BandCell& cell = g.cells[ci];
    const int first = ci ? g.cells[ci - 1].chunk_end : 0;
    const int ncx = (cell.w + CW - 1) / CW;
    const int lc = chunk - first;
    const int cx0 = (lc % ncx) * CW, cy0 = (lc / ncx) * CH;
    const int cw = min(CW, cell.w - cx0), ch = min(CH, cell.h - cy0);
    const int ax = cell.ox + cx0, ay = cell.oy + cy0;
    const int nt = cell.ntiles;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    for (int r = ty; r < ch; r += 16) {
        for (int x = tx; x < cw; x += 16) {
            const long long pix = (long long)(ay + r) * a.dst_row_stride + ax + x;
            float wv[MAX_COVER];
#pragma unroll
            for (int e = 0; e < MAX_COVER; ++e) {
                wv[e] = 0.f;
                if (e < nt) {
                    const int gt = cell.tile[e];
                    wv[e] = a.weight[(long long)(ay + r - g.tile_y[gt]) * a.W + ax + x - g.tile_x[gt]];
                }
            }
            const float nfull = a.norm_full[pix];
            for (int c0 = 0; c0 < a.C; c0 += CL_NC) {
                const int nc = min(CL_NC, a.C - c0);
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int e = 0; e < MAX_COVER; ++e) {
                    if (e < nt) {
                        const int gt = cell.tile[e];
                        cl_blend<OPK, IN, VEC>(a, static_cast<const float*>(g.tile_src[gt]), 0, g.tile_vs[gt], ay + r - g.tile_y[gt], ax + x - g.tile_x[gt], c0,
                                               nc, wv[e], acc);
                    }
                }
                cl_store_planes(a.merged + (long long)c0 * a.dst_chan_stride + pix, a.dst_chan_stride, nc, cl_div(acc, nfull));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ a launch group of a band plan (band_plan_kernel)
// blockIdx.x = work item of the plan's table (64 columns x 32 or 64 rows, <= 4 covering tiles in integration order); plain loop, no prefetch.
template <int OPK, int IN, bool VEC>
__global__ __launch_bounds__(CL_THREADS) void cl_plan_kernel(const ViewArgs a, const BandItem* __restrict__ items, const GroupTiles t) {
    const BandItem* __restrict__ it = items + blockIdx.x;
    const int cwch = it->cwch, partial = it->partial, nt = it->ntiles;
    const int cw = cwch & 0xffff, ch = cwch >> 16;
    const int ax = it->ax, ay = it->ay;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    for (int r = ty; r < ch; r += 16) {
        for (int x = tx; x < cw; x += 16) {
            const long long pix = (long long)(ay + r) * a.dst_row_stride + ax + x;
            float wv[MAX_COVER];
#pragma unroll
            for (int e = 0; e < MAX_COVER; ++e) {
                wv[e] = 0.f;
                if (e < nt) {
                    const unsigned long long cv = it->cover[e];
                    const int lx = (int)((cv >> 16) & 0xffff), ly = (int)((cv >> 32) & 0xffff);
                    wv[e] = a.weight[(long long)(ly + r) * a.W + lx + x];
                }
            }
            // the normaliser: the window values in integration order, as ptb_norm_accumulate sums them -- or the caller's map (a.norm_map: band_plan_kernel)
            float nsum = (a.norm_map && !partial) ? a.norm_full[pix] : 0.f;
#pragma unroll
            for (int e = 0; e < MAX_COVER; ++e)
                if (e < nt && !a.norm_map) nsum = __fadd_rn(nsum, wv[e]);
            for (int c0 = 0; c0 < a.C; c0 += CL_NC) {
                const int nc = min(CL_NC, a.C - c0);
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int e = 0; e < MAX_COVER; ++e) {
                    if (e < nt) {
                        const unsigned long long cv = it->cover[e];
                        const int slot = (int)(cv & 0xffff), lx = (int)((cv >> 16) & 0xffff), ly = (int)((cv >> 32) & 0xffff);
                        cl_blend<OPK, IN, VEC>(a, static_cast<const float*>(t.src[slot]), 0, t.vs[slot], ly + r, lx + x, c0, nc, wv[e], acc);
                    }
                }
                // (partial sums -- multi-GPU boundary rows -- are stored un-normalised, like band_plan_kernel)
                cl_store_planes(a.merged + (long long)c0 * a.dst_chan_stride + pix, a.dst_chan_stride, nc, partial ? acc : cl_div(acc, nsum));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ dispatch
// (linear | non-linear reduction) x source dtype x (vector | element loads): 12 instances per kernel, view codes and C at run time
template <class F>
static void with_cl_instance(const ViewArgs& a, bool vec, F&& f) {
    with_reduction(a.op, [&](auto opk) { with_src_dtype(a.in_dtype, [&](auto ld) { with_bool(vec, [&](auto v) {
        f(opk, int_c<ld_dtype<ld()>()>{}, v); }); }); });
}

// four channels per load: C a multiple of 4 (then every pixel of an aligned tile is aligned) and 16- / 8-byte aligned tiles.
// (Unlike cl3_vec_ok of the 3-D unit this does not look at g_force_scalar: known, and left as it is.)
static bool cl_vec_ok(const ViewArgs& a, const void* p, long long stride0, long long stride1) {
    const uintptr_t mask = a.in_dtype == PTB_F32 ? 15u : 7u;
    return a.C % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & mask) == 0 && stride0 % 4 == 0 && stride1 % 4 == 0;
}

void cl_launch_reduce(const ViewArgs& a, int ntiles_out, int ch, hipStream_t s) {
    const dim3 grid((unsigned)ntiles_out * a.chunks_x * a.chunks_y);
    const bool vec = cl_vec_ok(a, a.src, a.src_tile_stride, a.src_view_stride);
    with_cl_instance(a, vec, [&](auto opk, auto in, auto v) {
        hipLaunchKernelGGL((cl_reduce_kernel<opk(), in(), v()>), grid, dim3(CL_THREADS), 0, s, a, ch); });
}

void cl_launch_accum(const ViewArgs& a, const CellArgs& g, int ch, hipStream_t s) {
    const dim3 grid((unsigned)a.total_chunks);
    const bool vec = cl_vec_ok(a, a.src, a.src_tile_stride, a.src_view_stride);
    with_cl_instance(a, vec, [&](auto opk, auto in, auto v) {
        hipLaunchKernelGGL((cl_accum_kernel<opk(), in(), v()>), grid, dim3(CL_THREADS), 0, s, a, g, ch); });
}

void cl_launch_band(const ViewArgs& a, const BandArgs& g, int chunks, hipStream_t s) {
    const dim3 grid((unsigned)chunks);
    bool vec = true;
    for (int ci = 0; ci < a.ncells; ++ci)
        for (int e = 0; e < g.cells[ci].ntiles; ++e) vec = vec && cl_vec_ok(a, g.tile_src[g.cells[ci].tile[e]], g.tile_vs[g.cells[ci].tile[e]], 0);
    with_cl_instance(a, vec, [&](auto opk, auto in, auto v) {
        hipLaunchKernelGGL((cl_band_kernel<opk(), in(), v()>), grid, dim3(CL_THREADS), 0, s, a, g); });
}

void cl_launch_plan(const ViewArgs& a, const BandItem* items, const GroupTiles& t, int n_items, hipStream_t s) {
    const dim3 grid((unsigned)n_items);
    bool vec = true;
    for (int k = 0; k < PLAN_TILES; ++k)
        if (t.src[k]) vec = vec && cl_vec_ok(a, t.src[k], t.vs[k], 0);
    with_cl_instance(a, vec, [&](auto opk, auto in, auto v) {
        hipLaunchKernelGGL((cl_plan_kernel<opk(), in(), v()>), grid, dim3(CL_THREADS), 0, s, a, items, t); });
}

}  // namespace ptb
