// Launch arguments of the 3-D mirror TTA kernels (ptb_volume_tta.hip) and of the deferred slab merge (ptb_volume_bands.hip), defined
// here, not next to those kernels, because the channels-last kernels of ptb_volume_channels_last.hip consume them unchanged.
#pragma once
#include "ptb_view_device.h"

namespace ptb {

// ------------------------------------------------------------------------------------------------ mirror TTA (ptb_volume_tta.hip)
struct MirrorArgs {
    const void* src;
    void* dst;
    long long view_stride;  // elements between consecutive views in src (B * C * D * H * W); 0: src is the [B, C, ...] batch
    int B, C, D, H, W;
    int nv, masks;          // views, 3 bits each
    int op;                 // PTB_RED_* (reduce)
    float divisor;          // 1 for sum, V otherwise (reduce)
};

struct MirrorAccArgs {
    float* volume;        // [C, D', H', W']
    float* norm;          // [D', H', W']
    const float* weight;  // [d, h, w]
    const void* tiles;    // [V * B, C, d, h, w] of the source type
    long long view_stride;
    long long tile_off;   // element offset of tile b, view 0
    int C, d, h, w, D, H, W;
    int z0, y0, x0;
    int nv, masks, op;
    float divisor;
};

// ------------------------------------------------------------------------------------------------ deferred slab merge (ptb_volume_bands.hip)
constexpr int VB_COVER = 8;      // tiles covering one cell (half overlap on three axes)
constexpr int VB_TILES = 224;    // tiles of one launch group (kernarg: 224 x 16 B + VolArgs < 4 KiB)
constexpr int VB_BLOCK = 256;
constexpr int VB_UNITS = 1024;   // 4-runs per work item aimed at: four per lane

struct VolItem {                 // 96 B, read with scalar loads only
    int x0, y0, z0;              // origin in the padded volume (y, z clipped to the result window; x to its 4-aligned hull)
    int nx, ny, nz;
    int ntiles;                  // covering tiles (0: nobody covers these voxels -> 0 / 0 like the plain merge)
    int zero;                    // 0, as a value the compiler cannot fold (the dividend and divisor of an uncovered voxel)
    unsigned long long cover[VB_COVER];   // integration order: group slot | lx << 16 | ly << 32 | lz << 48 (item origin in the tile);
};                                        // entries past ntiles repeat entry 0 (a valid address for the unrolled loads)
static_assert(sizeof(VolItem) == 96, "VolItem layout");

struct VolTiles {
    const void* src[VB_TILES];   // view 0, channel 0 of the tile
    long long vs[VB_TILES];      // elements between consecutive views of this tile (its batch size * C * d * h * w)
};

struct VolArgs {
    const VolItem* items;        // first item of this launch
    const float* weight;         // [d, h, w]
    void* out;                   // the result window
    int C, d, h, w;
    int wz0, wy0, wx0, OD, OH, OW;
    int layout;                  // 0: [C, OD, OH, OW], 1: [OD, OH, OW, C] (argmax kinds: [OD, OH, OW])
    int nv, masks, op;           // mirror TTA: views, 3 bits each, PTB_RED_*
    float divisor;
};

template <int KIND>
constexpr bool vb_argmax() { return KIND == PTB_CROP_ARGMAX_U8 || KIND == PTB_CROP_ARGMAX_I64; }

// A lane's run of PIX voxels at padded (gz, gy, gx ..): the part of it inside the result window
struct VolPos { long long vox; int first, cnt; };   // window-linear index of the first stored voxel, its place in the run, how many
__device__ __forceinline__ VolPos vol_pos(const VolArgs& a, int gz, int gy, int gx, int npix) {
    const int lo = max(gx, a.wx0), hi = min(gx + npix, a.wx0 + a.OW);
    VolPos p;
    p.first = lo - gx;
    p.cnt = hi - lo;
    p.vox = ((long long)(gz - a.wz0) * a.OH + (gy - a.wy0)) * a.OW + (lo - a.wx0);
    return p;
}

// ------------------------------------------------------------------------------------------------ channels-last sources
// PTB_SRC_CHANNELS_LAST on a 5-D batch: `a.src` / `a.tiles` / the tile pointers address [.., d, h, w, C] memory (a model output in
// torch.channels_last_3d); everything else in the arguments means what it means to the planar kernels.  A lane owns one output voxel and
// walks its channels four at a time.  `dtype` = PTB_F32 | PTB_F16 | PTB_BF16 (the flag stripped).  Defined in ptb_volume_channels_last.hip.
void cl3_launch_reduce(const MirrorArgs& a, int dtype, hipStream_t s);                     // ptb_volume_mirror_reduce
void cl3_launch_accum(const MirrorAccArgs& a, int dtype, hipStream_t s);                   // ptb_volume_mirror_accumulate: tile a.tile_off
void cl3_launch_gather(const VolArgs& a, const VolTiles& t, int n_tiles, int dtype, int mode, int kind, int n_items,
                       hipStream_t s);                                                     // ptb_volume_plan_submit: one launch group

// ------------------------------------------------------------------------------------------------ activations
// One launch group of ptb_volume_plan_submit_act: the slab merge over A(tile) (PTB_ACT_*), dense or channels-last sources (`src_cl`).
// `dense_vec`: the dense criterion of the 4-voxel lanes holds (plan, weight and tile pointers on the 4-voxel grid).  Defined in
// ptb_volume_activation.hip.
void act_launch_gather(const VolArgs& a, const VolTiles& t, int n_tiles, int dtype, bool src_cl, bool dense_vec, int kind, int n_items,
                       int activation, float temperature, hipStream_t s);

}  // namespace ptb
