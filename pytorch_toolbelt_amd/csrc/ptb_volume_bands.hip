// ptb_volume_bands.hip -- the deferred slab merge of VolumeMerger(crops=, defer=True): the 3-D blend without accumulators.
//
// The crop list is known up front, so the host cuts every axis at all tile starts and ends: inside a CELL (a product of three
// intervals) the list of covering tiles is constant.  Cells that share a z-interval form a SLAB; the merger keeps references to the
// model outputs, and when the last tile over a slab is in, one launch reads every covering tile of every voxel of the slab, blends
// them in integration order in registers (acc = acc + t * w from +0, n = n + w: the accumulators' own sequence) and writes
// acc / n straight into the result window -- cast, layout and argmax as ptb_volume_merge_crop does them.  volume / norm_mask never
// exist, so nothing is read or written 8 times; voxels outside the result window are never computed.
//
//   * ptb_volume_plan_create / _items / _info: pure host code (testable without a device).
//   * ptb_volume_plan_upload / _submit / _reset / _state / _destroy: the per-image state machine, modelled on ptb_band_plan_*.
//
// A WORK ITEM is a box (cell x result window, cut into chunks of about 4096 voxels) = one workgroup; a lane owns 4 consecutive x of
// one row (16-byte tile and weight loads) or, where the x-origins, w or a pointer are off the 4-voxel grid, one voxel.  Tile reads
// are read-once (non-temporal), the window is re-read by every tile (ordinary loads).  Channels run in a loop with running argmax
// state, so registers do not depend on C.  No LDS, no scratch, no atomics.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ptb_crop_device.h"
#include "ptb_dispatch.h"
#include "ptb_mirror_device.h"
#include "ptb_volume_device.h"

namespace ptb {

// (VB_* constants, VolItem / VolTiles / VolArgs, vb_argmax and vol_pos: ptb_volume_device.h)

// v[m] <- v[m + s] (s in 0..3) with compile-time register indices
template <typename T>
__device__ __forceinline__ void shift4(T (&v)[4], int s) {
    if (s == 1) { v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; }
    else if (s == 2) { v[0] = v[2]; v[1] = v[3]; }
    else if (s == 3) { v[0] = v[3]; }
}

// Channel c of a run is ready: store it (cast and layout of ptb_merge_crop.hip), or fold it into the running argmax (first maximum
// wins; NaN counts as the maximum, like numpy / torch argmax)
template <int KIND, int PIX>
__device__ __forceinline__ void emit_channel(const VolArgs& a, const VolPos& p, int c, float (&q)[4], float (&best)[4], int (&arg)[4]) {
    if constexpr (vb_argmax<KIND>()) {
#pragma unroll
        for (int m = 0; m < PIX; ++m) {
            const bool take = c == 0 ? true : (q[m] > best[m] || (q[m] != q[m] && best[m] == best[m]));
            best[m] = take ? q[m] : best[m];
            arg[m] = take ? c : arg[m];
        }
    } else {
        if (p.cnt <= 0) return;
        if constexpr (PIX == 4) shift4(q, p.first);
        if (a.layout == 0 || a.C == 1) {
            store_out<KIND>(a.out, c * ((long long)a.OD * a.OH * a.OW) + p.vox, q, p.cnt);
        } else {
#pragma unroll
            for (int m = 0; m < PIX; ++m) {
                if (m < p.cnt) {
                    const float one[4] = {q[m], 0.f, 0.f, 0.f};
                    store_out<KIND>(a.out, (p.vox + m) * a.C + c, one, 1);
                }
            }
        }
    }
}

template <int KIND, int PIX>
__device__ __forceinline__ void emit_argmax(const VolArgs& a, const VolPos& p, int (&arg)[4]) {
    if constexpr (vb_argmax<KIND>()) {
        if (p.cnt <= 0) return;
        if constexpr (PIX == 4) shift4(arg, p.first);
        if constexpr (KIND == PTB_CROP_ARGMAX_U8) {
            uint8_t b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) b[m] = (uint8_t)arg[m];
            store_u8x4(static_cast<uint8_t*>(a.out) + p.vox, b, p.cnt);
        } else {
            long long* o = static_cast<long long*>(a.out) + p.vox;
#pragma unroll
            for (int m = 0; m < PIX; ++m)
                if (m < p.cnt) o[m] = arg[m];
        }
    }
}

// unit u of an item (PIX-runs, x fastest, then y, then z) -> offsets from the item's origin
template <int PIX>
__device__ __forceinline__ void unit_pos(int u, int xq, int ny, int& dz, int& dy, int& dx) {
    const int row = u / xq;
    dx = (u - row * xq) * PIX;
    dz = row / ny;
    dy = row - dz * ny;
}

__device__ __forceinline__ float4 weight_run4(const float* w, long long off) { return *reinterpret_cast<const float4*>(w + off); }

// ------------------------------------------------------------------------------------------------ no TTA
// NT = the item's tile count rounded up to 1, 2, 4 or 8: a fixed unrolled set of loads per lane, all issued before the dependent add
// chain; the padding entries load tile 0 again (an L1 hit) and are left out of the sums by a select, never by a branch around a load.
template <int LD, int PIX, int KIND, int NT>
__device__ __forceinline__ void gather_plain(const VolArgs& a, const VolTiles& t, const VolItem* it, int ntiles) {
    const int nx = it->nx, ny = it->ny, nz = it->nz, x0 = it->x0, y0 = it->y0, z0 = it->z0;
    const int xq = (nx + PIX - 1) / PIX;
    const int units = nz * ny * xq;
    const long long tplane = (long long)a.d * a.h * a.w;
    const float* src[NT];
    int lx[NT], ly[NT], lz[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const unsigned long long cv = it->cover[k];
        src[k] = static_cast<const float*>(t.src[(int)(cv & 0xffffu)]);
        lx[k] = (int)((cv >> 16) & 0xffffu);
        ly[k] = (int)((cv >> 32) & 0xffffu);
        lz[k] = (int)(cv >> 48);
    }
    for (int u = threadIdx.x; u < units; u += VB_BLOCK) {
        int dz, dy, dx;
        unit_pos<PIX>(u, xq, ny, dz, dy, dx);
        const VolPos p = vol_pos(a, z0 + dz, y0 + dy, x0 + dx, min(PIX, nx - dx));
        int off[NT];
        float4 wt[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            off[k] = ((lz[k] + dz) * a.h + ly[k] + dy) * a.w + lx[k] + dx;
            if constexpr (PIX == 4) wt[k] = weight_run4(a.weight, off[k]);
            else wt[k] = make_float4(a.weight[off[k]], 0.f, 0.f, 0.f);
        }
        float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const bool on = k < ntiles;
            n.x = on ? __fadd_rn(n.x, wt[k].x) : n.x; n.y = on ? __fadd_rn(n.y, wt[k].y) : n.y;
            n.z = on ? __fadd_rn(n.z, wt[k].z) : n.z; n.w = on ? __fadd_rn(n.w, wt[k].w) : n.w;
        }
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int arg[4] = {0, 0, 0, 0};
        for (int c = 0; c < a.C; ++c) {
            float4 v[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                if constexpr (PIX == 4) v[k] = ld4<LD>(src[k], c * tplane + off[k]);
                else v[k] = make_float4(widen<ld_dtype<LD>()>(src[k], c * tplane + off[k]), 0.f, 0.f, 0.f);
            }
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const bool on = k < ntiles;
                s.x = on ? __fadd_rn(s.x, __fmul_rn(v[k].x, wt[k].x)) : s.x; s.y = on ? __fadd_rn(s.y, __fmul_rn(v[k].y, wt[k].y)) : s.y;
                s.z = on ? __fadd_rn(s.z, __fmul_rn(v[k].z, wt[k].z)) : s.z; s.w = on ? __fadd_rn(s.w, __fmul_rn(v[k].w, wt[k].w)) : s.w;
            }
            float q[4] = {__fdiv_rn(s.x, n.x), __fdiv_rn(s.y, n.y), __fdiv_rn(s.z, n.z), __fdiv_rn(s.w, n.w)};
            emit_channel<KIND, PIX>(a, p, c, q, best, arg);
        }
        emit_argmax<KIND, PIX>(a, p, arg);
    }
}

// ------------------------------------------------------------------------------------------------ mirror TTA
// Per covering tile the V views are un-flipped and reduced by mirror_reduce_voxels (its loads issued before its sum), rounded to the
// source type (what ptb_volume_mirror_reduce stores) and blended; tiles are walked in a loop, the views are the unrolled set.
template <int LD, int OPK, int PIX, int KIND>
__device__ __forceinline__ void gather_tta(const VolArgs& a, const VolTiles& t, const VolItem* it, int ntiles) {
    const int nx = it->nx, ny = it->ny, nz = it->nz, x0 = it->x0, y0 = it->y0, z0 = it->z0;
    const int xq = (nx + PIX - 1) / PIX;
    const int units = nz * ny * xq;
    const long long tplane = (long long)a.d * a.h * a.w;
    for (int u = threadIdx.x; u < units; u += VB_BLOCK) {
        int dz, dy, dx;
        unit_pos<PIX>(u, xq, ny, dz, dy, dx);
        const VolPos p = vol_pos(a, z0 + dz, y0 + dy, x0 + dx, min(PIX, nx - dx));
        float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < ntiles; ++k) {
            const unsigned long long cv = it->cover[k];
            const int off = (((int)(cv >> 48) + dz) * a.h + (int)((cv >> 32) & 0xffffu) + dy) * a.w + (int)((cv >> 16) & 0xffffu) + dx;
            if constexpr (PIX == 4) {
                const float4 w4 = weight_run4(a.weight, off);
                n.x = __fadd_rn(n.x, w4.x); n.y = __fadd_rn(n.y, w4.y); n.z = __fadd_rn(n.z, w4.z); n.w = __fadd_rn(n.w, w4.w);
            } else {
                n.x = __fadd_rn(n.x, a.weight[off]);
            }
        }
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int arg[4] = {0, 0, 0, 0};
        for (int c = 0; c < a.C; ++c) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < ntiles; ++k) {
                const unsigned long long cv = it->cover[k];
                const int slot = (int)(cv & 0xffffu);
                const int tz = (int)(cv >> 48) + dz, ty = (int)((cv >> 32) & 0xffffu) + dy, tx = (int)((cv >> 16) & 0xffffu) + dx;
                const float4 r = mirror_reduce_voxels<LD, OPK, PIX>(t.src[slot], c * tplane, t.vs[slot], a.nv, a.masks, a.op, a.divisor, tz, ty,
                                                                    tx, a.d, a.h, a.w);
                const int off = (tz * a.h + ty) * a.w + tx;
                if constexpr (PIX == 4) {
                    const float4 w4 = weight_run4(a.weight, off);
                    s.x = __fadd_rn(s.x, __fmul_rn(round_src1<LD>(r.x), w4.x)); s.y = __fadd_rn(s.y, __fmul_rn(round_src1<LD>(r.y), w4.y));
                    s.z = __fadd_rn(s.z, __fmul_rn(round_src1<LD>(r.z), w4.z)); s.w = __fadd_rn(s.w, __fmul_rn(round_src1<LD>(r.w), w4.w));
                } else {
                    s.x = __fadd_rn(s.x, __fmul_rn(round_src1<LD>(r.x), a.weight[off]));
                }
            }
            float q[4] = {__fdiv_rn(s.x, n.x), 0.f, 0.f, 0.f};
            if constexpr (PIX == 4) { q[1] = __fdiv_rn(s.y, n.y); q[2] = __fdiv_rn(s.z, n.z); q[3] = __fdiv_rn(s.w, n.w); }
            emit_channel<KIND, PIX>(a, p, c, q, best, arg);
        }
        emit_argmax<KIND, PIX>(a, p, arg);
    }
}

// voxels nobody covers: what volume / norm_mask hold there is 0 and 0, and the plain merge divides them
template <int PIX, int KIND>
__device__ __forceinline__ void gather_empty(const VolArgs& a, const VolItem* it) {
    const int nx = it->nx, ny = it->ny, nz = it->nz;
    const int xq = (nx + PIX - 1) / PIX;
    const int units = nz * ny * xq;
    const float zero = __int_as_float(it->zero);
    for (int u = threadIdx.x; u < units; u += VB_BLOCK) {
        int dz, dy, dx;
        unit_pos<PIX>(u, xq, ny, dz, dy, dx);
        const VolPos p = vol_pos(a, it->z0 + dz, it->y0 + dy, it->x0 + dx, min(PIX, nx - dx));
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int arg[4] = {0, 0, 0, 0};
        for (int c = 0; c < a.C; ++c) {
            const float r = __fdiv_rn(zero, zero);
            float q[4] = {r, r, r, r};
            emit_channel<KIND, PIX>(a, p, c, q, best, arg);
        }
        emit_argmax<KIND, PIX>(a, p, arg);
    }
}

// LD: 1 = fp32, 2 = fp16, 3 = bf16 sources; MODE: 0 = plain tiles, 1 = mirror TTA with a linear reduction, 2 = with a non-linear one;
// PIX: 4-run | scalar lanes; KIND: PTB_CROP_*.  One workgroup per work item.
template <int LD, int MODE, int PIX, int KIND>
__global__ __launch_bounds__(VB_BLOCK) void volume_gather_kernel(const VolArgs a, const VolTiles t) {
    const VolItem* it = a.items + blockIdx.x;
    const int ntiles = it->ntiles;
    if (ntiles == 0) {
        gather_empty<PIX, KIND>(a, it);
    } else if constexpr (MODE == 0) {
        if (ntiles > 4) gather_plain<LD, PIX, KIND, 8>(a, t, it, ntiles);
        else if (ntiles > 2) gather_plain<LD, PIX, KIND, 4>(a, t, it, ntiles);
        else if (ntiles == 2) gather_plain<LD, PIX, KIND, 2>(a, t, it, ntiles);
        else gather_plain<LD, PIX, KIND, 1>(a, t, it, ntiles);
    } else {
        gather_tta<LD, MODE - 1, PIX, KIND>(a, t, it, ntiles);
    }
}

static void launch_gather(const VolArgs& a, const VolTiles& t, int in_dtype, int mode, bool vec, int kind, int n_items, hipStream_t s) {
    const dim3 grid((unsigned)n_items), block(VB_BLOCK);
    with_src_dtype(in_dtype, [&](auto ld) { with_value<0, 1, 2>(mode, [&](auto m) { with_bool(vec, [&](auto v) {
        with_crop_kind(kind, [&](auto k) {
            hipLaunchKernelGGL((volume_gather_kernel<ld(), m(), (v() ? 4 : 1), k()>), grid, block, 0, s, a, t); }); }); }); });
}

}  // namespace ptb

using namespace ptb;

// ------------------------------------------------------------------------------------------------ planning (host)
struct ptb_volume_plan {
    int n, C, d, h, w, D, H, W;
    int win[6];                       // z0, y0, x0, OD, OH, OW
    int layout, kind;
    std::vector<int64_t> zs, ys, xs;
    struct Group {
        int item0, n_items;           // range of `items`
        int z0, z1;                   // the slab's z-interval
        int complete;                 // the last tile (integration order) any of its items reads: launched once that tile is in
        std::vector<int> tiles;       // slot -> tile, ascending
    };
    std::vector<VolItem> items;       // launch order: groups by completing tile, heavy items first inside a group
    std::vector<int> item_tiles;      // VB_COVER per item: tile indices in integration order, -1 beyond ntiles
    std::vector<int> item_group;
    std::vector<Group> groups;
    std::vector<int> last_group;      // per tile: the last group that reads it, -1: none
    int n_slabs = 0, peak = 0;
    bool vec_ok = false;              // every x-origin and w on the 4-voxel grid: the 4-run instances may serve it
    const VolItem* dev_items = nullptr;
    // the image in flight
    int pos = 0, groups_done = 0;
    bool configured = false;
    int in_dtype = 0, nviews = 0, masks = 0, reduction = 0;
    bool act_entry = false;           // the image came in through ptb_volume_plan_submit_act
    int activation = 0;
    float temperature = 1.0f;
    const float* weight = nullptr;
    void* out = nullptr;
    std::vector<const void*> tile_src;
    std::vector<long long> tile_vs;
};

static std::vector<int> axis_cuts(const std::vector<int64_t>& starts, int size, int extent) {
    std::vector<int> c{0, extent};
    for (int64_t s : starts) { c.push_back((int)s); c.push_back((int)s + size); }
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    return c;
}

extern "C" int64_t ptb_volume_plan_create(const int64_t* zs, const int64_t* ys, const int64_t* xs, int n, int C, int d, int h, int w, int D,
                                          int H, int W, const int64_t* window, int layout, int kind, ptb_volume_plan** out) {
    if (!zs || !ys || !xs || !window || !out) return PTB_EINVAL;
    if (n < 1 || C < 1 || d < 1 || h < 1 || w < 1 || D < 1 || H < 1 || W < 1) return PTB_EINVAL;
    if (layout < 0 || layout > 1 || kind < PTB_CROP_F32 || kind > PTB_CROP_BF16) return PTB_EINVAL;
    for (int a = 0; a < 6; ++a)
        if (window[a] < 0) return PTB_EINVAL;
    if (window[0] + window[3] > D || window[1] + window[4] > H || window[2] + window[5] > W) return PTB_EBOUNDS;
    for (int t = 0; t < n; ++t)
        if (zs[t] < 0 || ys[t] < 0 || xs[t] < 0 || zs[t] + d > D || ys[t] + h > H || xs[t] + w > W) return PTB_EBOUNDS;
    if (kind == PTB_CROP_ARGMAX_U8 && C > 256) return PTB_EUNSUPPORTED;
    if (d > 0xffff || h > 0xffff || w > 0xffff || (long long)d * h * w > 0x7fffffffLL) return PTB_EUNSUPPORTED;   // the cover word, int offsets

    ptb_volume_plan* p = new ptb_volume_plan();
    p->n = n; p->C = C; p->d = d; p->h = h; p->w = w; p->D = D; p->H = H; p->W = W;
    for (int a = 0; a < 6; ++a) p->win[a] = (int)window[a];
    p->layout = layout; p->kind = kind;
    p->zs.assign(zs, zs + n); p->ys.assign(ys, ys + n); p->xs.assign(xs, xs + n);
    p->vec_ok = w % 4 == 0;
    for (int t = 0; t < n; ++t) p->vec_ok = p->vec_ok && xs[t] % 4 == 0;
    p->tile_src.assign(n, nullptr);
    p->tile_vs.assign(n, 0);
    p->last_group.assign(n, -1);

    const int wz0 = p->win[0], wy0 = p->win[1], wx0 = p->win[2];
    const int wz1 = wz0 + p->win[3], wy1 = wy0 + p->win[4], wx1 = wx0 + p->win[5];
    const int hx0 = wx0 & ~3, hx1 = (wx1 + 3) & ~3;      // the window's 4-aligned hull in x: the 4-run lanes stay on the tiles' 16-byte grid
    const std::vector<int> cz = axis_cuts(p->zs, d, D), cy = axis_cuts(p->ys, h, H), cx = axis_cuts(p->xs, w, W);

    struct Pending { VolItem item; int tiles[VB_COVER]; };
    std::vector<Pending> pending;          // items of the group being filled
    std::vector<int> group_tiles;          // its tiles
    std::vector<int> stamp(n, -1);         // tile -> the group (by serial number) that already lists it
    int serial = 0;
    bool too_many = false;
    std::vector<ptb_volume_plan::Group> groups;
    std::vector<std::vector<Pending>> group_items;
    int slab_z0 = 0, slab_z1 = 0;

    auto close_group = [&]() {
        if (!pending.empty()) {
            ptb_volume_plan::Group g;
            g.item0 = 0; g.n_items = (int)pending.size(); g.z0 = slab_z0; g.z1 = slab_z1;
            std::sort(group_tiles.begin(), group_tiles.end());
            g.tiles = group_tiles;
            g.complete = group_tiles.empty() ? 0 : group_tiles.back();
            std::stable_sort(pending.begin(), pending.end(), [](const Pending& a, const Pending& b) { return a.item.ntiles > b.item.ntiles; });
            groups.push_back(g);
            group_items.push_back(pending);
        }
        pending.clear();
        group_tiles.clear();
        ++serial;
    };

    std::vector<int> in_z, in_zy;
    for (size_t zi = 0; zi + 1 < cz.size() && !too_many; ++zi) {
        const int z0 = std::max(cz[zi], wz0), z1 = std::min(cz[zi + 1], wz1);
        if (z0 >= z1) continue;
        slab_z0 = cz[zi]; slab_z1 = cz[zi + 1];
        ++p->n_slabs;
        in_z.clear();
        for (int t = 0; t < n; ++t)
            if (zs[t] <= cz[zi] && cz[zi + 1] <= zs[t] + d) in_z.push_back(t);
        for (size_t yi = 0; yi + 1 < cy.size() && !too_many; ++yi) {
            const int y0 = std::max(cy[yi], wy0), y1 = std::min(cy[yi + 1], wy1);
            if (y0 >= y1) continue;
            in_zy.clear();
            for (int t : in_z)
                if (ys[t] <= cy[yi] && cy[yi + 1] <= ys[t] + h) in_zy.push_back(t);
            for (size_t xi = 0; xi + 1 < cx.size(); ++xi) {
                if (std::max(cx[xi], wx0) >= std::min(cx[xi + 1], wx1)) continue;
                const int x0 = std::max(cx[xi], hx0), x1 = std::min(cx[xi + 1], hx1);
                int cover[VB_COVER], nc = 0;
                for (int t : in_zy) {
                    if (xs[t] <= cx[xi] && cx[xi + 1] <= xs[t] + w) {
                        if (nc == VB_COVER) { too_many = true; break; }
                        cover[nc++] = t;
                    }
                }
                if (too_many) break;
                int fresh = 0;
                for (int k = 0; k < nc; ++k) fresh += stamp[cover[k]] != serial;
                if ((int)group_tiles.size() + fresh > VB_TILES) close_group();
                for (int k = 0; k < nc; ++k) {
                    if (stamp[cover[k]] != serial) { stamp[cover[k]] = serial; group_tiles.push_back(cover[k]); }
                }
                // cell x window, cut into boxes of about VB_UNITS 4-runs: whole rows, then whole planes
                const int nx = x1 - x0, ny = y1 - y0, nz = z1 - z0;
                const int rows = std::max(1, VB_UNITS / ((nx + 3) / 4));
                const int cy_ = std::min(ny, rows), cz_ = cy_ == ny ? std::max(1, rows / ny) : 1;
                for (int bz = z0; bz < z1; bz += cz_) {
                    for (int by = y0; by < y1; by += cy_) {
                        Pending q{};
                        q.item.x0 = x0; q.item.y0 = by; q.item.z0 = bz;
                        q.item.nx = nx; q.item.ny = std::min(cy_, y1 - by); q.item.nz = std::min(cz_, z1 - bz);
                        q.item.ntiles = nc;
                        for (int k = 0; k < VB_COVER; ++k) q.tiles[k] = k < nc ? cover[k] : -1;
                        pending.push_back(q);
                    }
                }
                (void)nz;
            }
        }
        close_group();       // a launch never spans two slabs: each is due at its own tile
    }
    if (too_many) { delete p; return PTB_EUNSUPPORTED; }

    // launch order: by completing tile (stable: slabs of one completing tile keep their z order)
    std::vector<int> order(groups.size());
    for (size_t g = 0; g < groups.size(); ++g) order[g] = (int)g;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return groups[a].complete < groups[b].complete; });
    std::vector<int> slot_of(n, 0);
    for (size_t gi = 0; gi < order.size(); ++gi) {
        ptb_volume_plan::Group g = groups[order[gi]];
        g.item0 = (int)p->items.size();
        for (size_t s = 0; s < g.tiles.size(); ++s) { slot_of[g.tiles[s]] = (int)s; p->last_group[g.tiles[s]] = (int)gi; }
        for (const Pending& q : group_items[order[gi]]) {
            VolItem it = q.item;
            for (int k = 0; k < VB_COVER; ++k) {
                const int t = q.tiles[k < it.ntiles ? k : 0];
                it.cover[k] = t < 0 ? 0ull
                                    : (unsigned long long)slot_of[t] | ((unsigned long long)(it.x0 - xs[t]) << 16) |
                                          ((unsigned long long)(it.y0 - ys[t]) << 32) | ((unsigned long long)(it.z0 - zs[t]) << 48);
                p->item_tiles.push_back(q.tiles[k]);
            }
            p->items.push_back(it);
            p->item_group.push_back((int)gi);
        }
        p->groups.push_back(g);
    }
    // tiles in custody, tile by tile: tile s is held from its own arrival until the tile that completes its last group is in
    std::vector<int> delta(n + 1, 0);
    for (int s = 0; s < n; ++s) {
        const int until = p->last_group[s] < 0 ? s : std::max(s, p->groups[p->last_group[s]].complete);
        delta[s] += 1;
        delta[until + 1] -= 1;
    }
    int held = 0;
    for (int s = 0; s < n; ++s) { held += delta[s]; p->peak = std::max(p->peak, held); }
    *out = p;
    return (int64_t)(p->items.size() * sizeof(VolItem));
}

extern "C" int64_t ptb_volume_plan_items(const ptb_volume_plan* p, int64_t* rows, int64_t capacity) {
    if (!p) return PTB_EINVAL;
    const int64_t n_items = (int64_t)p->items.size();
    if (!rows) return n_items;
    if (capacity < n_items) return PTB_EINVAL;
    const int wx0 = p->win[2], wx1 = p->win[2] + p->win[5];
    for (int64_t i = 0; i < n_items; ++i) {
        const VolItem& it = p->items[i];
        int64_t* r = rows + 16 * i;
        r[0] = p->item_group[i];
        r[1] = it.z0; r[2] = it.z0 + it.nz;
        r[3] = it.y0; r[4] = it.y0 + it.ny;
        r[5] = std::max(it.x0, wx0); r[6] = std::min(it.x0 + it.nx, wx1);
        r[7] = it.ntiles;
        for (int k = 0; k < VB_COVER; ++k) r[8 + k] = p->item_tiles[VB_COVER * i + k];
    }
    return n_items;
}

extern "C" int ptb_volume_plan_info(const ptb_volume_plan* p, int* n_groups, int* n_slabs, int64_t* n_items, int64_t* last_group_of_tile,
                                    int64_t* group_info /* [4 * n_groups]: z0, z1, completing tile, items */, int* peak_held_tiles,
                                    int* vec_ok) {
    if (!p) return PTB_EINVAL;
    if (n_groups) *n_groups = (int)p->groups.size();
    if (n_slabs) *n_slabs = p->n_slabs;
    if (n_items) *n_items = (int64_t)p->items.size();
    if (last_group_of_tile) for (int t = 0; t < p->n; ++t) last_group_of_tile[t] = p->last_group[t];
    if (group_info) {
        for (size_t g = 0; g < p->groups.size(); ++g) {
            group_info[4 * g] = p->groups[g].z0; group_info[4 * g + 1] = p->groups[g].z1;
            group_info[4 * g + 2] = p->groups[g].complete; group_info[4 * g + 3] = p->groups[g].n_items;
        }
    }
    if (peak_held_tiles) *peak_held_tiles = p->peak;
    if (vec_ok) *vec_ok = p->vec_ok ? 1 : 0;
    return PTB_OK;
}

extern "C" int ptb_volume_plan_upload(ptb_volume_plan* p, void* dev_table, ptb_stream_t stream) {
    if (!p || !dev_table || (reinterpret_cast<uintptr_t>(dev_table) & 15u)) return PTB_EINVAL;
    if (!p->items.empty()) {
        const hipError_t e = hipMemcpyAsync(dev_table, p->items.data(), p->items.size() * sizeof(VolItem), hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    }
    p->dev_items = static_cast<const VolItem*>(dev_table);
    return PTB_OK;
}

extern "C" int ptb_volume_plan_reset(ptb_volume_plan* p) {
    if (!p) return PTB_EINVAL;
    p->pos = 0; p->groups_done = 0; p->configured = false;
    std::fill(p->tile_src.begin(), p->tile_src.end(), nullptr);
    return PTB_OK;
}

extern "C" int ptb_volume_plan_state(const ptb_volume_plan* p, int* pos, int* launched) {
    if (!p) return PTB_EINVAL;
    if (pos) *pos = p->pos;
    if (launched) *launched = p->groups_done;
    return PTB_OK;
}

extern "C" void ptb_volume_plan_destroy(ptb_volume_plan* p) { delete p; }

// ptb_volume_plan_submit (act_entry = false) and ptb_volume_plan_submit_act (true: the kernels of ptb_volume_activation.hip)
static int plan_submit(ptb_volume_plan* p, int pos, int B, const void* batch, int64_t tile_stride, int64_t view_stride, int in_dtype, int nviews,
                       const int* masks, int reduction, const float* weight, void* out, bool act_entry, int activation, float temperature,
                       ptb_stream_t stream) {
    if (!p || !batch || !weight || !out || B < 1 || tile_stride < 1) return PTB_EINVAL;
    const int dtype_arg = in_dtype;      // (with PTB_SRC_CHANNELS_LAST: part of the image's configuration)
    const bool src_cl = (in_dtype & PTB_SRC_CHANNELS_LAST) != 0;
    in_dtype &= ~PTB_SRC_CHANNELS_LAST;
    if (in_dtype < PTB_F32 || in_dtype > PTB_BF16 || nviews < 0 || nviews > MAX_VIEWS) return PTB_EINVAL;
    int packed = 0;
    if (nviews > 0) {
        if (!masks || view_stride < 1 || reduction < PTB_RED_SUM || reduction > PTB_RED_LOG1P) return PTB_EINVAL;
        for (int k = 0; k < nviews; ++k) {
            if (masks[k] < 0 || masks[k] > 7) return PTB_EINVAL;
            packed |= masks[k] << (3 * k);
        }
    } else {
        reduction = 0;
        view_stride = 0;
    }
    if (activation == PTB_ACT_SOFTMAX && p->C > 16) return PTB_EUNSUPPORTED; // the channels of a voxel are resident
    if (!p->dev_items) return PTB_EINVAL;                                   // ptb_volume_plan_upload comes first
    if (pos != p->pos || (long long)pos + B > p->n) return PTB_EUNSUPPORTED;   // off the planned sequence
    if (p->configured && (dtype_arg != p->in_dtype || nviews != p->nviews || packed != p->masks || reduction != p->reduction ||
                          weight != p->weight || out != p->out || act_entry != p->act_entry || activation != p->activation ||
                          temperature != p->temperature))
        return PTB_EUNSUPPORTED;                                            // one configuration per image
    p->configured = true;
    p->act_entry = act_entry; p->activation = activation; p->temperature = temperature;
    p->in_dtype = dtype_arg; p->nviews = nviews; p->masks = packed; p->reduction = reduction; p->weight = weight; p->out = out;
    const size_t es = in_dtype == PTB_F32 ? 4 : 2;
    for (int b = 0; b < B; ++b) {
        p->tile_src[pos + b] = static_cast<const char*>(batch) + (size_t)b * (size_t)tile_stride * es;
        p->tile_vs[pos + b] = view_stride;
    }
    p->pos = pos + B;

    VolArgs a{};
    a.weight = weight; a.out = out;
    a.C = p->C; a.d = p->d; a.h = p->h; a.w = p->w;
    a.wz0 = p->win[0]; a.wy0 = p->win[1]; a.wx0 = p->win[2]; a.OD = p->win[3]; a.OH = p->win[4]; a.OW = p->win[5];
    a.layout = p->layout;
    a.nv = nviews; a.masks = packed; a.op = reduction;
    a.divisor = reduction == PTB_RED_SUM ? 1.0f : (float)nviews;
    const int mode = nviews == 0 ? 0 : (reduction >= PTB_RED_GMEAN ? 2 : 1);
    if (act_entry && nviews == 0) { a.nv = 1; a.op = PTB_RED_SUM; }       // plain tiles: the identity view, summed (exact)
    const uintptr_t run_mask = in_dtype == PTB_F32 ? 15u : 7u;            // 4 elements per lane: 16 B of fp32, 8 B of fp16 / bf16
    int launches = 0;
    while (p->groups_done < (int)p->groups.size() && p->groups[p->groups_done].complete < p->pos) {
        const ptb_volume_plan::Group& g = p->groups[p->groups_done];
        VolTiles t{};
        bool vec = p->vec_ok && !g_force_scalar && aligned16(weight);
        for (size_t s = 0; s < g.tiles.size(); ++s) {
            t.src[s] = p->tile_src[g.tiles[s]];
            t.vs[s] = p->tile_vs[g.tiles[s]];
            vec = vec && (reinterpret_cast<uintptr_t>(t.src[s]) & run_mask) == 0 && t.vs[s] % 4 == 0;
        }
        a.items = p->dev_items + g.item0;
        hipStream_t s = (hipStream_t)stream;
        if (act_entry) {
            act_launch_gather(a, t, (int)g.tiles.size(), in_dtype, src_cl, vec, p->kind, g.n_items, activation, temperature, s);
        } else if (src_cl) {   // PTB_SRC_CHANNELS_LAST: the same work-item table, one lane per voxel over all channels
            cl3_launch_gather(a, t, (int)g.tiles.size(), in_dtype, mode, p->kind, g.n_items, s);
        } else {
            launch_gather(a, t, in_dtype, mode, vec, p->kind, g.n_items, s);
        }
        if (int rc = check_launch()) return rc;
        ++p->groups_done;
        ++launches;
    }
    return launches;
}

extern "C" int ptb_volume_plan_submit(ptb_volume_plan* p, int pos, int B, const void* batch, int64_t tile_stride, int64_t view_stride,
                                      int in_dtype, int nviews, const int* masks, int reduction, const float* weight, void* out,
                                      ptb_stream_t stream) {
    return plan_submit(p, pos, B, batch, tile_stride, view_stride, in_dtype, nviews, masks, reduction, weight, out, false, PTB_ACT_NONE, 1.0f,
                       stream);
}

extern "C" int ptb_volume_plan_submit_act(ptb_volume_plan* p, int pos, int B, const void* batch, int64_t tile_stride, int64_t view_stride,
                                          int in_dtype, int nviews, const int* masks, int reduction, const float* weight, void* out,
                                          int activation, float temperature, ptb_stream_t stream) {
    if (activation < PTB_ACT_NONE || activation > PTB_ACT_SOFTMAX || !std::isfinite(temperature)) return PTB_EINVAL;
    return plan_submit(p, pos, B, batch, tile_stride, view_stride, in_dtype, nviews, masks, reduction, weight, out, true, activation,
                       temperature, stream);
}
