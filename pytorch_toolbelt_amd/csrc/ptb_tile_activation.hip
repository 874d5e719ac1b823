// ptb_tile_activation.hip -- sigmoid / softmax of the model's logits inside the 2-D de-augmentation and the tile merges
// (tta.*_image_deaugment, TileMerger.integrate_batch / accumulate_single / integrate_batch_deaugment, incremental and deferred bands;
// activation=), gfx950 / MI355X.
//
// A(y) = (y.float() * temperature).sigmoid() | .softmax(dim=1) is applied to every view of every tile in registers, where the planar and
// channels-last kernels (ptb_views.hip, ptb_bandplan.hip, ptb_channels_last.hip) only widen the logit: each call here means its namesake
// there on A(y), a float32 tensor that never exists.  So the source counts as float32 (no PTB_ROUND_SRC), and the order of every sum is
// the namesake's: views in view order through red_pre / red_post, tile * window rounded and added in integration order, __fdiv_rn.
// The host tables of the namesakes (chunk grid, cells with their first-touch state, the band plan's work items) are consumed unchanged.
//
// Channels-last source ([V*B, th, tw, C] memory): a lane owns one output pixel and its (up to 16) contiguous channels, fetched from each
// view's mirrored / transposed position (ptb_channels_last.hip's work division) -- all C logits of a softmax are in the lane.  16- / 8-byte
// loads when C % 4 == 0 and the tiles are aligned, element loads otherwise.  Sigmoid walks the channels in groups of 16.  No LDS.
//
// Dense planar source ([V*B, C, th, tw]): A is pointwise in space, so A(view(y)) == view(A(y)) and the logits are activated at their RAW
// position, between gather_widen and gather_tail -- before the transposing views go through the LDS tiles.  A workgroup (512 threads,
// 64 columns x 32 rows, one float4 per lane and view) takes a chunk / work item for ALL channels; taller chunks (64-row band items,
// other chunk sizes) are walked 32 rows at a time.  Softmax needs, per view and raw pixel, the maximum and the reciprocal sum over the C
// channel planes: this unit SWEEPS the channel planes twice for them (2 x NV float4 of state), then reads every plane a third time for
// the value -- the second and third reads hit L2.  Keeping C x NV raw vectors resident instead (128 registers of fp32 for C = 4 with d4)
// would bound C by the register file and need an instance per C; the sweep serves every C <= 16 with one instance and no scratch.
// Both give the same bits: max first, exp(z - max) summed in channel order, each term times the reciprocal of the sum.  Because the
// softmax state belongs to a covering tile, the covering tiles are the OUTER loop and the channels the inner one: the running weighted
// sum of a pixel lives in the accumulator image (incremental) or in the result map itself (deferred bands: partial sums are stored there,
// re-read by the same lane for the next covering tile and divided with the last one) -- L2-resident lines of the workgroup's own pixels.
//
// Activation, temperature, reduction and C are wave-uniform run-time values; source dtype, layout, view set (dense) and vector loads
// (channels-last) are the template axes.  No atomics, no scratch.
#include <cmath>

#include "ptb_activation_device.h"
#include "ptb_dispatch.h"
#include "ptb_view_device.h"

namespace ptb {

namespace {

constexpr int TA_CH = 32;                  // rows a dense workgroup covers per pass
constexpr int TA_THREADS = 16 * TA_CH;
constexpr int TA_CL_THREADS = 256;         // 16 x 16 pixels per pass of a channels-last workgroup
constexpr int TA_CREG = 16;                // resident channels of a channels-last lane
constexpr int TA_MAX_SOFTMAX_C = 16;

template <int LD> struct TaIn { static constexpr int value = ld_dtype<LD>(); };

// ------------------------------------------------------------------------------------------------ dense planar pieces
template <class F>
__device__ __forceinline__ float4 ta_map(const float4 v, F&& f) { return make_float4(f(v.x), f(v.y), f(v.z), f(v.w)); }
template <class F>
__device__ __forceinline__ float4 ta_zip(const float4 a, const float4 b, F&& f) { return make_float4(f(a.x, b.x), f(a.y, b.y), f(a.z, b.z), f(a.w, b.w)); }

// this lane's float4 of view k of one (tile, channel plane), widened, as gather_tail wants it (a lane without work holds 1): the body of
// gather_load_raw / gather_widen for one view, so that a kernel decides how many views it keeps in flight
template <int NV, int CODES, int LD>
__device__ __forceinline__ float4 ta_load_view(int k, const float* __restrict__ src, long long plane, long long view_stride, int nv, int codes, int H,
                                               int W, int lx, int ly, int cw, int ch, int tid) {
    constexpr int QPR = TA_CH / 4;
    float4 v = make_float4(1.f, 1.f, 1.f, 1.f);
    if (k < (CODES >= 0 ? NV : nv)) {
        const int code = ((CODES >= 0 ? CODES : codes) >> (3 * k)) & 7;
        const long long p = plane + (long long)k * view_stride;
        if (!(code & 1)) {
            const int q = tid & 15, r = tid >> 4;
            if ((r < ch) && (4 * q < cw)) {
                const int i = ly + r, j = lx + 4 * q;
                const int row = (code & 2) ? H - 1 - i : i;
                const int col = (code & 4) ? W - 4 - j : j;
                const float4 t = widen4<LD>(ld4_raw<LD>(src, p + (long long)row * W + col));
                v = (code & 4) ? make_float4(t.w, t.z, t.y, t.x) : t;
            }
        } else {
            const int rr = tid / QPR, qq = tid % QPR;
            if ((rr < cw) && (4 * qq < ch)) {
                const int R0 = (code & 2) ? H - lx - cw : lx;      // H == W for transposing views
                const int C0 = (code & 4) ? W - ly - ch : ly;
                v = widen4<LD>(ld4_raw<LD>(src, p + (long long)(R0 + rr) * W + C0 + 4 * qq));
            }
        }
    }
    return v;
}

// ... of every view.  The eight-view instances (64 registers of softmax state) request FLIGHT views at a time: with all eight in flight
// they spill
template <int NV, int CODES, int LD, int FLIGHT = 4>
__device__ __forceinline__ void ta_load(float4 (&v)[NV], const float* __restrict__ src, long long plane, long long view_stride, int nv, int codes, int H,
                                        int W, int lx, int ly, int cw, int ch, int tid) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k] = ta_load_view<NV, CODES, LD>(k, src, plane, view_stride, nv, codes, H, W, lx, ly, cw, ch, tid);
        if constexpr (NV == 8) {
            if (k % FLIGHT == FLIGHT - 1 && k + 1 < NV) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// softmax state of one covering tile: m[k] = max_c z, rs[k] = 1 / sum_c exp(z - m) (channel order), per view and raw pixel of the lane
template <int NV, int CODES, int LD, int FLIGHT = 4>
__device__ __forceinline__ void ta_softmax_state(float4 (&m)[NV], float4 (&rs)[NV], const float* __restrict__ src, long long tile0, long long view_stride,
                                                 int nv, int codes, int H, int W, int C, int lx, int ly, int cw, int ch, int tid, float t) {
    const long long hw = (long long)H * W;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        m[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        rs[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        float4 v[NV];
        ta_load<NV, CODES, LD, FLIGHT>(v, src, tile0 + c * hw, view_stride, nv, codes, H, W, lx, ly, cw, ch, tid);
#pragma unroll
        for (int k = 0; k < NV; ++k) m[k] = ta_zip(m[k], v[k], [=](float mm, float x) { return fmaxf(mm, __fmul_rn(x, t)); });
    }
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        float4 v[NV];
        ta_load<NV, CODES, LD, FLIGHT>(v, src, tile0 + c * hw, view_stride, nv, codes, H, W, lx, ly, cw, ch, tid);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const float4 e = ta_zip(v[k], m[k], [=](float x, float mm) { return fast_exp(__fsub_rn(__fmul_rn(x, t), mm)); });
            rs[k] = ta_zip(rs[k], e, [](float s, float ee) { return __fadd_rn(s, ee); });
        }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) rs[k] = ta_map(rs[k], [](float s) { return fast_rcp(s); });
}

// reduced value of channel plane `plane` of one covering tile: load, activate at the raw position, transpose / reduce (gather_tail)
template <int NV, int CODES, int LD, int FLIGHT = 4>
__device__ __forceinline__ float4 ta_value(const float4 (&m)[NV], const float4 (&rs)[NV], const float* __restrict__ src, long long plane,
                                           long long view_stride, int nv, int codes, int H, int W, int lx, int ly, int cw, int ch, int op, float divisor,
                                           int act, float t, float* lds, int tid) {
    float4 v[NV];
    ta_load<NV, CODES, LD, FLIGHT>(v, src, plane, view_stride, nv, codes, H, W, lx, ly, cw, ch, tid);
    if (act == PTB_ACT_SIGMOID) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = ta_map(v[k], [=](float x) { return act_sigmoid(__fmul_rn(x, t)); });
    } else if (act == PTB_ACT_SOFTMAX) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const float4 e = ta_zip(v[k], m[k], [=](float x, float mm) { return fast_exp(__fsub_rn(__fmul_rn(x, t), mm)); });
            v[k] = ta_zip(e, rs[k], [](float ee, float r) { return __fmul_rn(ee, r); });
        }
    }
    // (the LDS tiles are reused by the next channel / covering tile: always the trailing barrier)
    if (op >= PTB_RED_GMEAN) return gather_tail<TA_CH, NV, CODES, 1>(v, nv, codes, cw, ch, op, divisor, lds, tid, true);
    return gather_tail<TA_CH, NV, CODES, 0>(v, nv, codes, cw, ch, op, divisor, lds, tid, true);
}

// The work item as SCALARS, read before the kernel's first store: these kernels store partial sums between covering tiles, after which
// the compiler may no longer read the item with scalar loads -- and everything derived from it (tile pointers, offsets) would be per-lane.
__device__ __forceinline__ unsigned ta_uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned ta_pick(int e, unsigned v0, unsigned v1, unsigned v2, unsigned v3) {
    return e == 0 ? v0 : (e == 1 ? v1 : (e == 2 ? v2 : v3));
}
// (plain values, no struct: the item must live in scalar registers)
#define TA_READ_ITEM(itp)                                                                                                           \
    const int it_ax = __builtin_amdgcn_readfirstlane((itp)->ax), it_ay = __builtin_amdgcn_readfirstlane((itp)->ay);                 \
    const int it_cwch = __builtin_amdgcn_readfirstlane((itp)->cwch);                                                                \
    const int nt = __builtin_amdgcn_readfirstlane((itp)->ntiles), partial = __builtin_amdgcn_readfirstlane((itp)->partial);         \
    const unsigned long long it_c0 = (itp)->cover[0], it_c1 = (itp)->cover[1], it_c2 = (itp)->cover[2], it_c3 = (itp)->cover[3];    \
    const unsigned it_lo0 = ta_uniform((unsigned)it_c0), it_hi0 = ta_uniform((unsigned)(it_c0 >> 32));                              \
    const unsigned it_lo1 = ta_uniform((unsigned)it_c1), it_hi1 = ta_uniform((unsigned)(it_c1 >> 32));                              \
    const unsigned it_lo2 = ta_uniform((unsigned)it_c2), it_hi2 = ta_uniform((unsigned)(it_c2 >> 32));                              \
    const unsigned it_lo3 = ta_uniform((unsigned)it_c3), it_hi3 = ta_uniform((unsigned)(it_c3 >> 32))
// cover entry e (run-time, wave-uniform) of the item: tile slot, item origin inside the tile
#define TA_COVER(e, slot, lx, ly)                                                       \
    const unsigned cv_lo = ta_pick(e, it_lo0, it_lo1, it_lo2, it_lo3);                  \
    const unsigned cv_hi = ta_pick(e, it_hi0, it_hi1, it_hi2, it_hi3);                  \
    const int slot = (int)(cv_lo & 0xffff), lx = (int)(cv_lo >> 16), ly = (int)(cv_hi & 0xffff)

__device__ __forceinline__ float4 ta_blend(const float4 acc, const float4 val, const float4 w) {   // tiles.py:338: product rounded, then added
    return make_float4(__fadd_rn(acc.x, __fmul_rn(val.x, w.x)), __fadd_rn(acc.y, __fmul_rn(val.y, w.y)), __fadd_rn(acc.z, __fmul_rn(val.z, w.z)),
                       __fadd_rn(acc.w, __fmul_rn(val.w, w.w)));
}
__device__ __forceinline__ float4 ta_div(const float4 s, const float4 n) {                          // tiles.py:346
    return make_float4(__fdiv_rn(s.x, n.x), __fdiv_rn(s.y, n.y), __fdiv_rn(s.z, n.z), __fdiv_rn(s.w, n.w));
}

template <int NV, int CODES>
constexpr int ta_lds_floats() { return lds_tiles(NV, CODES) ? lds_tiles(NV, CODES) * CW * TA_CH : 4; }

}  // namespace

// ------------------------------------------------------------------------------------------------ dense: de-augment + reduce
// out[t] = reduce_k(pre(A(view_k(src[k * B + t])))), dense fp32; blockIdx.x = (tile, 64 x 32 chunk), all channels
template <int NV, int CODES, int LD>
__global__ __launch_bounds__(TA_THREADS) void tact_reduce_kernel(const ViewArgs a, const int act, const float temp) {
    __shared__ __attribute__((aligned(16))) float lds[ta_lds_floats<NV, CODES>()];
    const int tid = threadIdx.x;
    const int cpt = a.chunks_x * a.chunks_y;
    const int chunk = blockIdx.x % cpt, t = blockIdx.x / cpt;
    const int cx0 = (chunk % a.chunks_x) * CW, cy0 = (chunk / a.chunks_x) * TA_CH;
    const int cw = min(CW, a.W - cx0), ch = min(TA_CH, a.H - cy0);
    const int q = tid & 15, r = tid >> 4;
    const bool lane = (r < ch) && (4 * q < cw);
    const long long tile0 = (long long)t * a.src_tile_stride, hw = (long long)a.H * a.W;
    float4 m[NV], rs[NV];
    if (act == PTB_ACT_SOFTMAX)
        ta_softmax_state<NV, CODES, LD>(m, rs, a.src, tile0, a.src_view_stride, a.nviews, a.codes, a.H, a.W, a.C, cx0, cy0, cw, ch, tid, temp);
    float* o = a.dst + (long long)t * a.dst_tile_stride + (long long)(cy0 + r) * a.dst_row_stride + cx0 + 4 * q;
#pragma unroll 1
    for (int c = 0; c < a.C; ++c) {
        const float4 val = ta_value<NV, CODES, LD>(m, rs, a.src, tile0 + c * hw, a.src_view_stride, a.nviews, a.codes, a.H, a.W, cx0, cy0, cw, ch, a.op,
                                                   a.divisor, act, temp, lds, tid);
        if (lane) out_store4(o + (long long)c * a.dst_chan_stride, val);
    }
}

// ------------------------------------------------------------------------------------------------ dense: accumulate (view_accum_kernel's cells)
// blockIdx.x = chunk (64 columns x `chrows` rows of a cell, all channels).  Covering tiles outside, channels inside: the accumulator
// element is read-modify-written once per covering tile (a first-touch cell starts its first tile from zero instead of reading).
template <int NV, int CODES, int LD>
__global__ __launch_bounds__(TA_THREADS) void tact_accum_kernel(const ViewArgs a, const CellArgs g, const int chrows, const int act, const float temp) {
    __shared__ __attribute__((aligned(16))) float lds[ta_lds_floats<NV, CODES>()];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x;
    int ci = 0;
    while (ci < a.ncells - 1 && chunk >= g.cells[ci].chunk_end) ++ci;
    const Cell& cell = g.cells[ci];
    const int first = ci ? g.cells[ci - 1].chunk_end : 0;
    const int ncx = (cell.w + CW - 1) / CW;
    const int lc = chunk - first;
    const int cx0 = (lc % ncx) * CW, cy0 = (lc / ncx) * chrows;
    const int cw = min(CW, cell.w - cx0), rows = min(chrows, cell.h - cy0);
    const int nt = cell.ntiles, fresh = cell.fresh;
    const int q = tid & 15, r = tid >> 4;
    const long long hw = (long long)a.H * a.W;
#pragma unroll 1
    for (int r0 = 0; r0 < rows; r0 += TA_CH) {
        const int ch = min(TA_CH, rows - r0);
        const int ax = cell.ox + cx0, ay = cell.oy + cy0 + r0;   // origin of this pass in the accumulator
        const bool lane = (r < ch) && (4 * q < cw);
        const long long pix = (long long)(ay + r) * a.dst_row_stride + ax + 4 * q;
        if (a.norm != nullptr && lane) {   // norm == NULL: the caller keeps the (data independent) normaliser itself
            float4 nacc = fresh ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(a.norm + pix);
            for (int e = 0; e < nt; ++e) {
                const int gt = cell.tile[e];
                const float4 w4 = *reinterpret_cast<const float4*>(a.weight + (long long)(ay - g.tile_y[gt] + r) * a.W + ax - g.tile_x[gt] + 4 * q);
                nacc = make_float4(__fadd_rn(nacc.x, w4.x), __fadd_rn(nacc.y, w4.y), __fadd_rn(nacc.z, w4.z), __fadd_rn(nacc.w, w4.w));
            }
            *reinterpret_cast<float4*>(a.norm + pix) = nacc;
        }
#pragma unroll 1
        for (int e = 0; e < nt; ++e) {
            const int gt = cell.tile[e];
            const int lx = ax - g.tile_x[gt], ly = ay - g.tile_y[gt];
            const long long tile0 = (long long)g.tile_id[gt] * a.src_tile_stride;
            float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane) w4 = *reinterpret_cast<const float4*>(a.weight + (long long)(ly + r) * a.W + lx + 4 * q);
            float4 m[NV], rs[NV];
            if (act == PTB_ACT_SOFTMAX)
                ta_softmax_state<NV, CODES, LD>(m, rs, a.src, tile0, a.src_view_stride, a.nviews, a.codes, a.H, a.W, a.C, lx, ly, cw, ch, tid, temp);
#pragma unroll 1
            for (int c = 0; c < a.C; ++c) {
                const float4 val = ta_value<NV, CODES, LD>(m, rs, a.src, tile0 + c * hw, a.src_view_stride, a.nviews, a.codes, a.H, a.W, lx, ly, cw, ch,
                                                           a.op, a.divisor, act, temp, lds, tid);
                if (lane) {
                    float* ip = a.dst + (long long)c * a.dst_chan_stride + pix;
                    const float4 acc = (fresh && e == 0) ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(ip);
                    *reinterpret_cast<float4*>(ip) = ta_blend(acc, val, w4);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ dense: a launch group of a band plan (band_plan_kernel's items)
// blockIdx.x = work item (64 columns x 32 or 64 rows, <= 4 covering tiles in integration order), all channels.  The weighted sum of a
// pixel is kept in the result map between covering tiles (plain stores, re-read by the same lane) and divided with the last one.
template <int NV, int CODES, int LD>
__global__ __launch_bounds__(TA_THREADS) void tact_plan_kernel(const ViewArgs a, const BandItem* __restrict__ items, const GroupTiles t, const int act,
                                                               const float temp) {
    __shared__ __attribute__((aligned(16))) float lds[ta_lds_floats<NV, CODES>()];
    const int tid = threadIdx.x;
    TA_READ_ITEM(items + blockIdx.x);
    const int cw = it_cwch & 0xffff, rows = it_cwch >> 16;
    const int q = tid & 15, r = tid >> 4;
    const long long hw = (long long)a.H * a.W;
    if (nt == 0) {   // uncovered pixels: 0 / 0 like the plain merge (a path of its own: inside the pass loop it cost the eight-view instances spills)
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        float nz = 0.f;                       // the sum of no window value, kept from the compiler: the division below is the hardware's,
        asm volatile("" : "+v"(nz));          // so the NaN carries the bits the plain merge's 0 / 0 has
        const float4 nsum = make_float4(nz, nz, nz, nz);
        for (int rr = r; rr < rows && 4 * q < cw; rr += TA_CH) {
            const long long pix = (long long)(it_ay + rr) * a.dst_row_stride + it_ax + 4 * q;
            for (int c = 0; c < a.C; ++c) {
                float* o = a.merged + (long long)c * a.dst_chan_stride + pix;
                if (partial) *reinterpret_cast<float4*>(o) = zero;
                else out_store4(o, ta_div(zero, nsum));
            }
        }
        return;
    }
#pragma unroll 1
    for (int r0 = 0; r0 < rows; r0 += TA_CH) {
        const int ch = min(TA_CH, rows - r0);
        const bool lane = (r < ch) && (4 * q < cw);
        const long long pix = (long long)(it_ay + r0 + r) * a.dst_row_stride + it_ax + 4 * q;
        float4 nsum = make_float4(0.f, 0.f, 0.f, 0.f);   // the normaliser: the window values in integration order (band_plan_kernel), complete with the last tile
#pragma unroll 1
        for (int e = 0; e < nt; ++e) {
            TA_COVER(e, slot, lx, ly0);
            const int ly = ly0 + r0;
            const float* __restrict__ src = static_cast<const float*>(t.src[slot]);
            const long long vs = t.vs[slot];
            float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane) w4 = *reinterpret_cast<const float4*>(a.weight + (long long)(ly + r) * a.W + lx + 4 * q);
            nsum = make_float4(__fadd_rn(nsum.x, w4.x), __fadd_rn(nsum.y, w4.y), __fadd_rn(nsum.z, w4.z), __fadd_rn(nsum.w, w4.w));
            float4 m[NV], rs[NV];
            if (act == PTB_ACT_SOFTMAX) ta_softmax_state<NV, CODES, LD>(m, rs, src, 0, vs, a.nviews, a.codes, a.H, a.W, a.C, lx, ly, cw, ch, tid, temp);
            const bool last = e + 1 == nt;
#pragma unroll 1
            for (int c = 0; c < a.C; ++c) {
                const float4 val = ta_value<NV, CODES, LD>(m, rs, src, c * hw, vs, a.nviews, a.codes, a.H, a.W, lx, ly, cw, ch, a.op, a.divisor, act, temp,
                                                           lds, tid);
                if (lane) {
                    float* o = a.merged + (long long)c * a.dst_chan_stride + pix;
                    const float4 acc = ta_blend(e ? *reinterpret_cast<const float4*>(o) : make_float4(0.f, 0.f, 0.f, 0.f), val, w4);
                    if (last && !partial) out_store4(o, ta_div(acc, nsum));
                    else *reinterpret_cast<float4*>(o) = acc;      // (partial sums are read back soon: plain store)
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ channels-last pieces
namespace {

// v[c][0] <- channels c0 + c (c < nc) of the pixel whose channel c0 is element `off` of `base`; the channels from nc to the end of the
// last group of four repeat channel nc - 1 (a valid address; see activate)
template <int LD, bool VEC>
__device__ __forceinline__ void tcl_load(float (&v)[TA_CREG][1], const float* __restrict__ base, long long off, int nc) {
#pragma unroll
    for (int g = 0; g < TA_CREG; g += 4) {
        if (g < nc) {
            if constexpr (VEC) {
                const float4 t = ld4<LD>(base, off + g);
                v[g][0] = t.x; v[g + 1][0] = t.y; v[g + 2][0] = t.z; v[g + 3][0] = t.w;
            } else {
#pragma unroll
                for (int c = g; c < g + 4; ++c) v[c][0] = widen<TaIn<LD>::value>(base, off + min(c, nc - 1));
            }
        }
    }
}

// r[c][0] = post(sum_k pre(A(view_k))) of channels c0 + c (c < nc) of output pixel (i, j) of one tile; `off0` = view 0 of the tile
template <int LD, bool VEC>
__device__ __forceinline__ void tcl_reduce_px(float (&r)[TA_CREG][1], const float* __restrict__ base, long long off0, long long view_stride, int nv,
                                              int codes, int H, int W, int C, int i, int j, int c0, int nc, int op, float divisor, int act, float t) {
#pragma unroll
    for (int c = 0; c < TA_CREG; ++c) r[c][0] = 0.f;
#pragma unroll 1
    for (int k = 0; k < nv; ++k) {
        const int code = (codes >> (3 * k)) & 7;      // out[i][j] = src[rr][cc]: the mapping of cl_reduce_px (ptb_channels_last.hip)
        int rr = (code & 1) ? j : i, cc = (code & 1) ? i : j;
        const int rows = (code & 1) ? W : H, cols = (code & 1) ? H : W;
        if (code & 2) rr = rows - 1 - rr;
        if (code & 4) cc = cols - 1 - cc;
        float v[TA_CREG][1];
        tcl_load<LD, VEC>(v, base, off0 + (long long)k * view_stride + ((long long)rr * cols + cc) * C + c0, nc);
        activate(v, nc, act, t);
        act_red_pre(v, nc, op);
        act_each(r, nc, [&](float s, int c, int) { return k ? __fadd_rn(s, v[c][0]) : v[c][0]; });
    }
    act_red_post(r, nc, op, divisor);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ channels-last: de-augment + reduce
template <int LD, bool VEC>
__global__ __launch_bounds__(TA_CL_THREADS) void tact_cl_reduce_kernel(const ViewArgs a, const int act, const float temp) {
    const int cpt = a.chunks_x * a.chunks_y;
    const int chunk = blockIdx.x % cpt, t = blockIdx.x / cpt;
    const int cx0 = (chunk % a.chunks_x) * CW, cy0 = (chunk / a.chunks_x) * TA_CH;
    const int cw = min(CW, a.W - cx0), ch = min(TA_CH, a.H - cy0);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long off0 = (long long)t * a.src_tile_stride;
    for (int r = ty; r < ch; r += 16) {
        for (int x = tx; x < cw; x += 16) {
            const int i = cy0 + r, j = cx0 + x;
            float* o = a.dst + (long long)t * a.dst_tile_stride + (long long)i * a.dst_row_stride + j;
            for (int c0 = 0; c0 < a.C; c0 += TA_CREG) {
                const int nc = min(TA_CREG, a.C - c0);
                float v[TA_CREG][1];
                tcl_reduce_px<LD, VEC>(v, a.src, off0, a.src_view_stride, a.nviews, a.codes, a.H, a.W, a.C, i, j, c0, nc, a.op, a.divisor, act, temp);
#pragma unroll
                for (int c = 0; c < TA_CREG; ++c)
                    if (c < nc) o[(long long)(c0 + c) * a.dst_chan_stride] = v[c][0];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ channels-last: accumulate
template <int LD, bool VEC>
__global__ __launch_bounds__(TA_CL_THREADS) void tact_cl_accum_kernel(const ViewArgs a, const CellArgs g, const int chrows, const int act, const float temp) {
    const int chunk = blockIdx.x;
    int ci = 0;
    while (ci < a.ncells - 1 && chunk >= g.cells[ci].chunk_end) ++ci;
    const Cell& cell = g.cells[ci];
    const int first = ci ? g.cells[ci - 1].chunk_end : 0;
    const int ncx = (cell.w + CW - 1) / CW;
    const int lc = chunk - first;
    const int cx0 = (lc % ncx) * CW, cy0 = (lc / ncx) * chrows;
    const int cw = min(CW, cell.w - cx0), ch = min(chrows, cell.h - cy0);
    const int ax = cell.ox + cx0, ay = cell.oy + cy0;
    const int nt = cell.ntiles, fresh = cell.fresh;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    for (int r = ty; r < ch; r += 16) {
        for (int x = tx; x < cw; x += 16) {
            const long long pix = (long long)(ay + r) * a.dst_row_stride + ax + x;
            if (a.norm != nullptr) {
                float nacc = fresh ? 0.f : a.norm[pix];
                for (int e = 0; e < nt; ++e) {
                    const int gt = cell.tile[e];
                    nacc = __fadd_rn(nacc, a.weight[(long long)(ay + r - g.tile_y[gt]) * a.W + ax + x - g.tile_x[gt]]);
                }
                a.norm[pix] = nacc;
            }
            for (int c0 = 0; c0 < a.C; c0 += TA_CREG) {
                const int nc = min(TA_CREG, a.C - c0);
                float* ip = a.dst + (long long)c0 * a.dst_chan_stride + pix;
                float s[TA_CREG][1];
#pragma unroll
                for (int c = 0; c < TA_CREG; ++c) s[c][0] = (fresh || c >= nc) ? 0.f : ip[(long long)c * a.dst_chan_stride];
#pragma unroll 1
                for (int e = 0; e < nt; ++e) {
                    const int gt = cell.tile[e];
                    const int li = ay + r - g.tile_y[gt], lj = ax + x - g.tile_x[gt];
                    const float w = a.weight[(long long)li * a.W + lj];
                    float v[TA_CREG][1];
                    tcl_reduce_px<LD, VEC>(v, a.src, (long long)g.tile_id[gt] * a.src_tile_stride, a.src_view_stride, a.nviews, a.codes, a.H, a.W, a.C, li,
                                           lj, c0, nc, a.op, a.divisor, act, temp);
                    act_each(s, nc, [&](float acc, int c, int) { return __fadd_rn(acc, __fmul_rn(v[c][0], w)); });
                }
#pragma unroll
                for (int c = 0; c < TA_CREG; ++c)
                    if (c < nc) ip[(long long)c * a.dst_chan_stride] = s[c][0];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ channels-last: a launch group of a band plan
template <int LD, bool VEC>
__global__ __launch_bounds__(TA_CL_THREADS) void tact_cl_plan_kernel(const ViewArgs a, const BandItem* __restrict__ items, const GroupTiles t, const int act,
                                                                     const float temp) {
    TA_READ_ITEM(items + blockIdx.x);
    const int cw = it_cwch & 0xffff, ch = it_cwch >> 16;
    const int ax = it_ax, ay = it_ay;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    for (int r = ty; r < ch; r += 16) {
        for (int x = tx; x < cw; x += 16) {
            const long long pix = (long long)(ay + r) * a.dst_row_stride + ax + x;
            float nsum = 0.f;   // the normaliser: summed from the window values beside the first channel group's blend (band_plan_kernel)
            for (int c0 = 0; c0 < a.C; c0 += TA_CREG) {
                const int nc = min(TA_CREG, a.C - c0);
                float s[TA_CREG][1];
#pragma unroll
                for (int c = 0; c < TA_CREG; ++c) s[c][0] = 0.f;
#pragma unroll 1
                for (int e = 0; e < nt; ++e) {
                    TA_COVER(e, slot, lx, ly);
                    const int lj = lx + x, li = ly + r;
                    const float w = a.weight[(long long)li * a.W + lj];
                    if (c0 == 0) nsum = __fadd_rn(nsum, w);
                    float v[TA_CREG][1];
                    tcl_reduce_px<LD, VEC>(v, static_cast<const float*>(t.src[slot]), 0, t.vs[slot], a.nviews, a.codes, a.H, a.W, a.C, li, lj, c0, nc, a.op,
                                           a.divisor, act, temp);
                    act_each(s, nc, [&](float acc, int c, int) { return __fadd_rn(acc, __fmul_rn(v[c][0], w)); });
                }
                float* o = a.merged + (long long)c0 * a.dst_chan_stride + pix;
#pragma unroll
                for (int c = 0; c < TA_CREG; ++c)
                    if (c < nc) o[(long long)c * a.dst_chan_stride] = partial ? s[c][0] : __fdiv_rn(s[c][0], nsum);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ dispatch
namespace {

// dense: view set x source dtype (18 instances per kernel); channels-last: source dtype x (vector | element loads) (6 per kernel)
// (no instance with the view codes read at run time: it would spill next to the softmax state.  A view set that is none of the TTA
// groups is not served here -- ta_view_set_ok -- and the caller applies A itself)
template <class F>
void with_ta_dense(const ViewArgs& a, F&& f) {
    with_view_set(a.nviews, a.codes, [&](auto nv, auto codes) { with_src_dtype(a.in_dtype, [&](auto ld) {
        if constexpr (codes() >= 0) f(nv, codes, ld);
        else no_instance("ptb_tile_activation");
    }); });
}
template <class F>
void with_ta_cl(const ViewArgs& a, bool vec, F&& f) {
    with_src_dtype(a.in_dtype, [&](auto ld) { with_bool(vec, [&](auto v) { f(ld, v); }); });
}

// four channels per load: C a multiple of 4 (then every pixel of an aligned tile is aligned) and 16- / 8-byte aligned tiles
bool ta_cl_vec(const ViewArgs& a, const void* p, long long stride0, long long stride1) {
    const uintptr_t mask = a.in_dtype == PTB_F32 ? 15u : 7u;
    return !g_force_scalar && a.C % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & mask) == 0 && stride0 % 4 == 0 && stride1 % 4 == 0;
}

}  // namespace

// planar sources: the view sets with compiled-in codes -- identity and the five TTA groups
bool ta_view_set_ok(int nviews, int codes) {
    bool ok = false;
    with_view_set(nviews, codes, [&](auto, auto c) { ok = c() >= 0; });
    return ok;
}

void ta_launch_accum(const ViewArgs& a, const CellArgs& g, int ch, bool src_cl, int activation, float temperature, hipStream_t s) {
    const dim3 grid((unsigned)a.total_chunks);
    if (src_cl) {
        with_ta_cl(a, ta_cl_vec(a, a.src, a.src_tile_stride, a.src_view_stride), [&](auto ld, auto v) {
            hipLaunchKernelGGL((tact_cl_accum_kernel<ld(), v()>), grid, dim3(TA_CL_THREADS), 0, s, a, g, ch, activation, temperature); });
    } else {
        with_ta_dense(a, [&](auto nv, auto codes, auto ld) {
            hipLaunchKernelGGL((tact_accum_kernel<nv(), codes(), ld()>), grid, dim3(TA_THREADS), 0, s, a, g, ch, activation, temperature); });
    }
}

void ta_launch_plan(const ViewArgs& a, const BandItem* items, const GroupTiles& t, int n_items, bool src_cl, int activation, float temperature,
                    hipStream_t s) {
    const dim3 grid((unsigned)n_items);
    if (src_cl) {
        bool vec = true;
        for (int k = 0; k < PLAN_TILES; ++k)
            if (t.src[k]) vec = vec && ta_cl_vec(a, t.src[k], t.vs[k], 0);
        with_ta_cl(a, vec, [&](auto ld, auto v) {
            hipLaunchKernelGGL((tact_cl_plan_kernel<ld(), v()>), grid, dim3(TA_CL_THREADS), 0, s, a, items, t, activation, temperature); });
    } else {
        with_ta_dense(a, [&](auto nv, auto codes, auto ld) {
            hipLaunchKernelGGL((tact_plan_kernel<nv(), codes(), ld()>), grid, dim3(TA_THREADS), 0, s, a, items, t, activation, temperature); });
    }
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_deaug_reduce_act(const void* in, int in_dtype, float* out, int V, const int* views, int reduction, int B, int C, int H, int W,
                                    int activation, float temperature, ptb_stream_t stream) {
    const bool src_cl = (in_dtype & PTB_SRC_CHANNELS_LAST) != 0;
    in_dtype &= ~PTB_SRC_CHANNELS_LAST;
    if (in_dtype < PTB_F32 || in_dtype > PTB_BF16) return PTB_EINVAL;
    if (!in || !out || B < 0 || C < 1 || H < 1 || W < 1) return PTB_EINVAL;
    if (reduction < PTB_RED_SUM || reduction > PTB_RED_LOG1P) return PTB_EINVAL;
    if (activation < PTB_ACT_NONE || activation > PTB_ACT_SOFTMAX || !std::isfinite(temperature)) return PTB_EINVAL;
    if (V < 1 || V > MAX_VIEWS || !views) return PTB_EINVAL;
    int nT = 0, codes = 0;
    for (int k = 0; k < V; ++k) {
        if (views[k] < 0 || views[k] > 7) return PTB_EINVAL;
        nT += views[k] & 1;
        codes |= views[k] << (3 * k);
    }
    if (nT && H != W) return PTB_EINVAL;
    if (activation == PTB_ACT_SOFTMAX && C > TA_MAX_SOFTMAX_C) return PTB_EUNSUPPORTED;
    // the planar vector kernels' shapes (run_plain of ptb_views.hip): everything on the 4-pixel grid; channels-last lanes own a pixel
    const bool aligned_src = (reinterpret_cast<uintptr_t>(in) & (in_dtype == PTB_F32 ? 15u : 7u)) == 0;
    const bool fast = !g_force_scalar && W % 4 == 0 && aligned_src && aligned16(out) && nT <= MAX_T && !(nT && H % 4 != 0);
    if (!src_cl && (!fast || !ta_view_set_ok(V, codes))) return PTB_EUNSUPPORTED;
    if (B == 0) return PTB_OK;
    ViewArgs a{};
    a.src = static_cast<const float*>(in); a.dst = out;
    a.in_dtype = in_dtype;
    a.H = H; a.W = W; a.C = C;
    a.src_view_stride = (long long)B * C * H * W;
    a.src_tile_stride = (long long)C * H * W;
    a.dst_tile_stride = (long long)C * H * W;
    a.dst_chan_stride = (long long)H * W;
    a.dst_row_stride = W;
    a.nviews = V;
    a.codes = codes;
    a.scale = 1.0f;
    a.op = reduction;
    a.divisor = reduction == PTB_RED_SUM ? 1.0f : (float)V;
    a.chunks_x = (W + CW - 1) / CW;
    a.chunks_y = (H + TA_CH - 1) / TA_CH;
    const long long blocks = (long long)B * a.chunks_x * a.chunks_y;
    if (blocks > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    const dim3 grid((unsigned)blocks);
    hipStream_t s = (hipStream_t)stream;
    if (src_cl) {
        with_ta_cl(a, ta_cl_vec(a, a.src, a.src_tile_stride, a.src_view_stride), [&](auto ld, auto v) {
            hipLaunchKernelGGL((tact_cl_reduce_kernel<ld(), v()>), grid, dim3(TA_CL_THREADS), 0, s, a, activation, temperature); });
    } else {
        with_ta_dense(a, [&](auto nv, auto codes_c, auto ld) {
            hipLaunchKernelGGL((tact_reduce_kernel<nv(), codes_c(), ld()>), grid, dim3(TA_THREADS), 0, s, a, activation, temperature); });
    }
    return check_launch();
}
