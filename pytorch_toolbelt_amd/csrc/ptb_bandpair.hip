// ptb_bandpair.hip -- the deferred band merge of fp16 / bf16 d4 model outputs on PAIRS of work items (gfx950 / MI355X).
//
// band_plan_kernel (ptb_bandplan.hip) reads a 64 x 64 block per workgroup.  Of a 16-bit plane that is 64 row segments of 128 bytes for
// every view -- and for the four TRANSPOSING d4 views the other 128 bytes of each 256-byte stretch belong to the item 64 rows further
// down, a workgroup dispatched an item row later (profiles/r06_band_half_diag.txt: 16 % of the image's time; fp32 sources read 256-byte
// segments either way and do not pay it).  The plan therefore puts vertically adjacent items next to each other in its table
// (BandItem::pair_top), and this kernel takes such a couple as ONE 64 x 128 block: the transposing views are read in 64 source rows of
// 256 bytes, 16 bytes per lane, the row-preserving ones as before (two 8-byte loads per lane, rows r and r + 64).  Everything after the
// loads is band_plan_kernel's arithmetic per half -- views summed in view order, rounded, blended in integration order, the normaliser
// summed from the window values -- so the bits are the same.  Not served here: normaliser maps (rank launches), fused activations,
// channels-last sources, other view sets, fp32: they keep band_plan_kernel on the same table.
#include "ptb_dispatch.h"
#include "ptb_view_device.h"

namespace ptb {

typedef unsigned int raw4 __attribute__((ext_vector_type(4)));

constexpr int PAIR_SET = lds_tiles(8, CODES_D4) * CW * 64;      // floats of one half's four transposed tiles (64 KiB)

// swzg (ptb_view_device.h) with the 16-byte slots of the BOTTOM half's tiles (hb = 1) shifted by one: lanes q and q + 8 of a source row
// scatter the same (row, column) of the two halves, 64 KiB apart -- on one bank without the shift.
__device__ __forceinline__ int pair_slot(int i, int slot, int hb) { return i * CW + (((slot ^ (i >> 2) ^ hb) & 15) << 2); }
__device__ __forceinline__ int pair_swz(int i, int j, int hb) { return pair_slot(i, j >> 2, hb) + ((j & 3) ^ ((i >> 4) & 2)); }

template <int OPK, int LD>
__global__ __launch_bounds__(1024) void band_pair_kernel(const ViewArgs a, const BandItem* __restrict__ items, const GroupTiles t) {
    constexpr int NV = 8, CODES = CODES_D4;
    __shared__ __attribute__((aligned(16))) float lds[2 * PAIR_SET];      // the top half's tiles, then the bottom half's
    const int tid = threadIdx.x;
    const unsigned bid = blockIdx.x;
    const int c = bid % a.C;
    const BandItem* __restrict__ it = items + 2 * (size_t)(bid / a.C);   // the top item; the bottom one differs in ay and ly only (+ 64)
    const int cw = it->cwch & 0xffff, partial = it->partial, nt = it->ntiles;
    // (r, 4q) is this lane's pixel quad in either half AND its place in the transposing views' source block: row r, columns 8q .. 8q + 7
    const int q = tid & 15, r = tid >> 4;
    const bool act = 4 * q < cw, tact = r < cw;
    const int H = a.H, W = a.W;      // (H == W: the tile is square)
    // Every address is a wave-uniform base (tile, view, channel, the block's corner: scalar registers) plus one of six per-lane offsets
    // that no covering tile changes -- row r or its mirror 63 - r, quad 4q or its mirror 60 - 4q; source row r, columns 8q .. 8q + 7; the window -- kept in
    // BYTES: a 32-bit offset that is added unscaled is what the load's scalar-base form takes.
    // Lanes outside a narrow item (cw < 64) load what lane q = 0 / r = 0 loads instead of nothing: every load is then unconditional, the
    // compiler counts the ones in flight exactly, and no address leaves the block.
    const int ql = act ? q : 0, rl = tact ? r : 0;
    const unsigned lane_rp[2][2] = {{2u * (r * W + 4 * ql), 2u * (r * W + 60 - 4 * ql)},
                                    {2u * ((63 - r) * W + 4 * ql), 2u * ((63 - r) * W + 60 - 4 * ql)}};      // [rows mirrored][columns mirrored]
    const unsigned lane_tr = 2u * (rl * W + 8 * q), lane_w = 4u * (r * W + 4 * ql);

    raw2 rp[2][NV];                  // row-preserving views of the covering tile in flight, [half][view], as they lie in memory
    raw4 tr[NV];                     // transposing views: eight source columns, all of one half
    float4 wn;                       // the top half's window values: they travel with the views
    auto request = [&](int e) {
        const unsigned long long cv = it->cover[e];
        const int slot = (int)(cv & 0xffff), lx = (int)((cv >> 16) & 0xffff), ly = (int)((cv >> 32) & 0xffff);
        const unsigned short* __restrict__ src = static_cast<const unsigned short*>(t.src[slot]) + (long long)c * H * W;
        const long long vs = t.vs[slot];
        // (the offsets pass through an empty asm so that their widening to 64 bits stays next to the loads: hoisted out of the tile loop it
        // turns every load of the loop into the two-register address form, twelve registers instead of six)
        unsigned orp[2][2] = {{lane_rp[0][0], lane_rp[0][1]}, {lane_rp[1][0], lane_rp[1][1]}}, otr = lane_tr, ow = lane_w;
        asm volatile("" : "+v"(orp[0][0]), "+v"(orp[0][1]), "+v"(orp[1][0]), "+v"(orp[1][1]), "+v"(otr), "+v"(ow));
        const float* wbase = a.weight + (long long)ly * W + lx;
        wn = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(wbase) + ow);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int code = (CODES >> (3 * k)) & 7;
            const unsigned short* view = src + (long long)k * vs;
            if (code & 1) {
                const int R0 = (code & 2) ? H - lx - cw : lx;
                const int C0 = (code & 4) ? W - ly - 128 : ly;
                tr[k] = __builtin_nontemporal_load(reinterpret_cast<const raw4*>(reinterpret_cast<const char*>(view + (long long)R0 * W + C0) + otr));
            } else {
                const int col0 = (code & 4) ? W - 64 - lx : lx;      // the block's first column in memory
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int row0 = (code & 2) ? H - 64 - (ly + 64 * h) : ly + 64 * h;      // ... and this half's first row
                    rp[h][k] = __builtin_nontemporal_load(reinterpret_cast<const raw2*>(reinterpret_cast<const char*>(view + (long long)row0 * W + col0) +
                                                                                        orp[(code >> 1) & 1][(code >> 2) & 1]));
                }
            }
        }
    };

    float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    float4 nsum[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    request(0);                      // (a pair has at least one covering tile)
    for (int e = 0; e < nt; ++e) {
        // transposing views: source row r is output column r (mirrored under code & 2), source columns 8q .. 8q + 7 are eight output rows of
        // ONE half -- columns 0 .. 63 of the block are the top half's rows, 64 .. 127 the bottom half's; mirrored, hence swapped, under code & 4
        if (tact) {
            int tb = 0;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int code = (CODES >> (3 * k)) & 7;
                if (!(code & 1)) continue;
                const int hb = (q >> 3) ^ ((code >> 2) & 1);
                const int qe = (code & 4) ? 7 - (q & 7) : (q & 7);      // the lane's eight output rows are 8qe .. 8qe + 7 of half hb, in reverse when mirrored
                const int jl = (code & 2) ? cw - 1 - r : r;
                // TWO addresses per view, the rest immediate offsets (32 separate ones were hoisted out of the loop and spilled): rows 8qe .. 8qe + 3
                // keep column jl in one 16-byte slot, rows 8qe + 4 .. 8qe + 7 in its neighbour (the swizzle's row term advances by one)
                const int at = pair_swz(8 * qe, jl, hb);
                float* buf = lds + hb * PAIR_SET + tb * (CW * 64);
                ++tb;
                const float4 lo = widen4<LD>(raw2{tr[k].x, tr[k].y}), hi = widen4<LD>(raw2{tr[k].z, tr[k].w});
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const int sm = (code & 4) ? 7 - m : m;               // source column 8q + sm lands in row 8qe + m
                    buf[(m < 4 ? at : at ^ 4) + m * CW] = sm < 4 ? comp(lo, sm) : comp(hi, sm - 4);
                }
            }
        }
        raw2 cur[2][NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) { cur[0][k] = rp[0][k]; cur[1][k] = rp[1][k]; }
        // (the bottom half's window values are requested HERE, in front of the next tile: the four registers they would hold across the
        // reduction are the ones the kernel does not have -- the table is 1 MiB, served by the L2, and loads return in order)
        const unsigned long long cv = it->cover[e];
        const float4 w4[2] = {wn, *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.weight + (long long)((int)((cv >> 32) & 0xffff) + 64) * W +
                                                                                                   (int)((cv >> 16) & 0xffff)) + lane_w)};
        if (e + 1 < nt) request(e + 1);      // (the raw registers are free again: the next covering tile travels while this one is reduced)
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float4 v[NV];
            int tb = 0;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int code = (CODES >> (3 * k)) & 7;
                if (code & 1) {
                    const float* buf = lds + h * PAIR_SET + tb * (CW * 64);
                    ++tb;
                    v[k] = unswz4(*reinterpret_cast<const float4*>(buf + pair_slot(r, q, h)), r);
                } else {
                    const float4 x = widen4<LD>(cur[h][k]);
                    v[k] = (code & 4) ? make_float4(x.w, x.z, x.y, x.x) : x;
                }
            }
            float4 val = reduce_views<NV, OPK>(v, NV, a.op, a.divisor);
            val = round_src4<LD>(val, a.round_src);
            acc[h].x = __fadd_rn(acc[h].x, __fmul_rn(val.x, w4[h].x));   // tiles.py:338: tile * weight rounded, then added (no FMA contraction)
            acc[h].y = __fadd_rn(acc[h].y, __fmul_rn(val.y, w4[h].y));
            acc[h].z = __fadd_rn(acc[h].z, __fmul_rn(val.z, w4[h].z));
            acc[h].w = __fadd_rn(acc[h].w, __fmul_rn(val.w, w4[h].w));
            nsum[h].x = __fadd_rn(nsum[h].x, w4[h].x);                   // tiles.py:339: the normaliser's own sum, same order
            nsum[h].y = __fadd_rn(nsum[h].y, w4[h].y);
            nsum[h].z = __fadd_rn(nsum[h].z, w4[h].z);
            nsum[h].w = __fadd_rn(nsum[h].w, w4[h].w);
        }
        if (e + 1 < nt) __syncthreads();     // the tiles are scattered again
    }
    if (act) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float* o = a.merged + (long long)c * a.dst_chan_stride + (long long)(it->ay + 64 * h + r) * a.dst_row_stride + it->ax + 4 * q;
            if (partial) *reinterpret_cast<float4*>(o) = acc[h];          // (partial sums are read back soon: plain store)
            else out_store4(o, make_float4(__fdiv_rn(acc[h].x, nsum[h].x), __fdiv_rn(acc[h].y, nsum[h].y), __fdiv_rn(acc[h].z, nsum[h].z),
                                           __fdiv_rn(acc[h].w, nsum[h].w)));   // tiles.py:346
        }
    }
}

void bp_launch_pairs(const ViewArgs& a, const BandItem* items, const GroupTiles& t, int pairs, hipStream_t s) {
    const dim3 grid((unsigned)pairs * (unsigned)a.C), block(1024);
    with_reduction(a.op, [&](auto opk) { with_src_dtype(a.in_dtype, [&](auto ld) {
        if constexpr (ld() >= 2) hipLaunchKernelGGL((band_pair_kernel<opk(), ld()>), grid, block, 0, s, a, items, t);
        else no_instance("band_pair_kernel");
    }); });
}

int g_band_pairs = 1;      // ptb_set_tunable key 28: fp16 / bf16 d4 band launches take the paired items of a group through band_pair_kernel

}  // namespace ptb
