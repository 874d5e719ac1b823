// ptb_volume_resample.hip -- trilinear resampling of a volume before the 3-D tiled-inference loop:
//
//   * ptb_volume_resize_trilinear: .float() + F.interpolate(mode="trilinear") + .to(half) of a [D, H, W(, C)] volume of any element type
//     ptb_volume_split reads -- a scan brought to the spacing the model was trained at, with no float32 copy of the input.
//
// An HBM-bound gather, no MFMA.  A workgroup of 256 threads owns an output brick of 64 x 4 x 4 (x, y, z), x running over the RW * C
// elements of a channel-last row; a lane owns 4 consecutive x elements of one row, so stores are 16 B (fp32) / 8 B (half) per lane.  The
// source sub-brick the taps of the brick read is staged in LDS, widened to fp32: each source voxel is loaded once per workgroup instead
// of once per tap, and the 8 taps of an output are LDS reads.  When the largest source brick of a launch exceeds the LDS brick (strong
// down-sampling) the launch gathers straight from global memory instead (STAGE = false), as the tiled multiscale kernel of
// ptb_resample.hip falls back per scale.
//
// Taps: ptb_taps_device.h, the arithmetic of the 2-D resize kernels.  Blend order x, y, z; -ffp-contract=off keeps every product and
// sum rounded on its own, which is what the float32 restatement of the tests evaluates.
#include <algorithm>

#include "ptb_crop_device.h"   // store_out: 4 consecutive fp32 / fp16 / bf16 outputs
#include "ptb_dispatch.h"
#include "ptb_taps_device.h"

namespace ptb {

constexpr int VR_TX = 64, VR_TY = 4, VR_TZ = 4;     // output brick of a workgroup
constexpr int VR_ROWS = VR_TY * VR_TZ / 16;         // rows (y, z) per lane: 16 lanes span the 64 x outputs, 16 rows go in parallel
constexpr int VR_ZSTEP = 16 / VR_TY;                // ... so a lane's rows are VR_ZSTEP planes apart
constexpr int VR_BRICK = 2560;                      // floats of the source brick in LDS (10 KiB; x 1.5 up-sampling needs 44 x 5 x 5)
constexpr int VR_PER = VR_BRICK / 256;              // brick elements a lane stages
constexpr int MAX_VRESIZE_C = 16;

struct VRArgs {
    const void* vol;     // [D, H, W, C] of the input type
    void* out;           // [RD, RH, RW, C]
    long long sY, sZ;    // elements between source rows / planes (W * C, H * W * C)
    int C;               // channels, interleaved along x
    int ID, IH, IW;      // source extent in voxels
    int RD, RH, RW;      // output extent in voxels
    float sd, sh, sw;    // scales of the three axes
    int align;
    int tiles_x, tiles_y;
};

// source voxels [lo, lo + n) that the taps of outputs first .. last read (i0 and i1 do not decrease with the output index)
struct Span { int lo, n; };
__device__ __forceinline__ Span span(int first, int last, float scale, int n_in, bool ac) {
    const int lo = taps(first, scale, n_in, ac).i0;
    return {lo, taps(last, scale, n_in, ac).i1 - lo + 1};
}

// A lane's taps as brick-relative element offsets: 4 consecutive x elements, one y, VR_ROWS z -- into the LDS brick, or (direct launches)
// into global memory behind the brick's first voxel; 32 bits either way (the host checks).  l = the weight of the second tap; the first
// one's, 1 - l, is evaluated at its use.  Indexed by unrolled constants only: registers, no scratch.
struct LaneTaps {
    unsigned x0[4], xd[4];
    float xl[4];
    unsigned y0, y1;
    float yl;
    unsigned z0[VR_ROWS], z1[VR_ROWS];
    float zl[VR_ROWS];
};

// xc: elements per voxel along x (the channels of a channel-last volume); e0: the lane's first x element of RWe; the lane's
// rows are (oy, oz + VR_ZSTEP * j).  Outputs past the edge take the taps of the last output (inside the brick; they are never stored).
__device__ __forceinline__ void lane_taps(LaneTaps& L, const VRArgs& a, int xc, int e0, int RWe, int oy, int oz, Span bx, Span by, Span bz,
                                          unsigned sy, unsigned sz, bool ac) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int e = min(e0 + m, RWe - 1), x = e / xc, ch = e - x * xc;
        const Taps t = taps(x, a.sw, a.IW, ac);
        L.x0[m] = (unsigned)((t.i0 - bx.lo) * xc + ch);
        L.xd[m] = (unsigned)((t.i1 - t.i0) * xc);
        L.xl[m] = t.l1;
    }
    const Taps ty = taps(min(oy, a.RH - 1), a.sh, a.IH, ac);
    L.y0 = (unsigned)(ty.i0 - by.lo) * sy; L.y1 = (unsigned)(ty.i1 - by.lo) * sy;
    L.yl = ty.l1;
#pragma unroll
    for (int j = 0; j < VR_ROWS; ++j) {
        const Taps tz = taps(min(oz + VR_ZSTEP * j, a.RD - 1), a.sd, a.ID, ac);
        L.z0[j] = (unsigned)(tz.i0 - bz.lo) * sz; L.z1[j] = (unsigned)(tz.i1 - bz.lo) * sz;
        L.zl[j] = tz.l1;
    }
}

// the lane's 4 outputs of row j: x first (a * (1 - lx) + b * lx), then the rows with ly, then the planes with lz
template <class F>
__device__ __forceinline__ void lerp_row(const LaneTaps& L, int j, F&& fetch, float* res) {
    const float yl0 = 1.f - L.yl, zl0 = 1.f - L.zl[j];
    const unsigned r00 = L.z0[j] + L.y0, r01 = L.z0[j] + L.y1, r10 = L.z1[j] + L.y0, r11 = L.z1[j] + L.y1;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const unsigned i0 = L.x0[m], i1 = L.x0[m] + L.xd[m];
        const float xl0 = 1.f - L.xl[m], xl1 = L.xl[m];
        const float t00 = fetch(r00 + i0) * xl0 + fetch(r00 + i1) * xl1;
        const float t01 = fetch(r01 + i0) * xl0 + fetch(r01 + i1) * xl1;
        const float t10 = fetch(r10 + i0) * xl0 + fetch(r10 + i1) * xl1;
        const float t11 = fetch(r11 + i0) * xl0 + fetch(r11 + i1) * xl1;
        const float p0 = t00 * yl0 + t01 * L.yl;
        const float p1 = t10 * yl0 + t11 * L.yl;
        res[m] = p0 * zl0 + p1 * L.zl[j];
    }
}

// Global offsets (behind the brick's first voxel) of the brick elements e = tid + 256 k a lane stages; the brick is nx elements wide and
// ny rows high, `total` elements in all (<= VR_BRICK, and its last offset fits 32 bits: the host checks both).  Elements past the brick
// read offset 0.
__device__ __forceinline__ void stage_offsets(int tid, int nx, int ny, int total, long long sY, long long sZ, unsigned (&off)[VR_PER]) {
    const int drow = 256 / nx, dx = 256 - drow * nx, dz = drow / ny, dy = drow - dz * ny;
    const int row = tid / nx;
    int x = tid - row * nx, z = row / ny;
    int y = row - z * ny;
#pragma unroll
    for (int k = 0; k < VR_PER; ++k) {
        off[k] = tid + 256 * k < total ? (unsigned)(z * sZ + y * sY + x) : 0u;
        x += dx; y += dy; z += dz;
        if (x >= nx) { x -= nx; ++y; }
        if (y >= ny) { y -= ny; ++z; }
    }
}

struct BrickTile { int ox0, oy0, oz0; };
__device__ __forceinline__ BrickTile brick_tile(const VRArgs& a) {
    int b = blockIdx.x;
    const int tx = b % a.tiles_x;
    b /= a.tiles_x;
    return {tx * VR_TX, (b % a.tiles_y) * VR_TY, (b / a.tiles_y) * VR_TZ};
}

// ------------------------------------------------------------------------------------------------ resize of a channel-last volume
// x runs over the RW * C elements of an output row, a lane's 4 consecutive elements take the taps of their voxels, and the LDS brick
// holds whole source voxels (widened to fp32 on load).
template <int IN, int OUT, bool STAGE>
__global__ __launch_bounds__(256) void volume_resize_kernel(const VRArgs a) {
    constexpr int KIND = OUT == PTB_F32 ? PTB_CROP_F32 : (OUT == PTB_F16 ? PTB_CROP_F16 : PTB_CROP_BF16);
    __shared__ float qb[STAGE ? VR_BRICK : 1];
    const int tid = threadIdx.x;
    const bool ac = a.align != 0;
    const int C = a.C, RWe = a.RW * C;
    const BrickTile t = brick_tile(a);
    const Span bx = span(t.ox0 / C, (min(t.ox0 + VR_TX, RWe) - 1) / C, a.sw, a.IW, ac);
    const Span by = span(t.oy0, min(t.oy0 + VR_TY, a.RH) - 1, a.sh, a.IH, ac);
    const Span bz = span(t.oz0, min(t.oz0 + VR_TZ, a.RD) - 1, a.sd, a.ID, ac);
    const int nxe = bx.n * C;
    const unsigned sy = STAGE ? (unsigned)nxe : (unsigned)a.sY, sz = STAGE ? (unsigned)(nxe * by.n) : (unsigned)a.sZ;
    const int e0 = t.ox0 + 4 * (tid & 15), oy = t.oy0 + ((tid >> 4) & (VR_TY - 1)), oz = t.oz0 + (tid >> 4) / VR_TY;
    LaneTaps L;
    lane_taps(L, a, C, e0, RWe, oy, oz, bx, by, bz, sy, sz, ac);
    const int nv = oy < a.RH ? max(0, min(4, RWe - e0)) : 0;
    const long long borg = bz.lo * a.sZ + by.lo * a.sY + (long long)bx.lo * C;
    if constexpr (STAGE) {
        const int total = nxe * by.n * bz.n;
        unsigned off[VR_PER];
        stage_offsets(tid, nxe, by.n, total, a.sY, a.sZ, off);
#pragma unroll
        for (int k = 0; k < VR_PER; ++k) {
            const float v = widen<IN>(a.vol, borg + off[k]);
            if (tid + 256 * k < total) qb[tid + 256 * k] = v;
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < VR_ROWS; ++j) {
        float res[4];
        if constexpr (STAGE) lerp_row(L, j, [&](unsigned i) { return qb[i]; }, res);
        else lerp_row(L, j, [&](unsigned i) { return widen<IN>(a.vol, borg + i); }, res);
        if (nv > 0 && oz + VR_ZSTEP * j < a.RD) store_out<KIND>(a.out, ((long long)(oz + VR_ZSTEP * j) * a.RH + oy) * RWe + e0, res, nv);
    }
}

// ------------------------------------------------------------------------------------------------ host side
static float axis_scale(int n_in, int n_out, int align_corners) {
    if (align_corners) return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
    return (float)n_in / (float)n_out;
}

// The widest source span of any tile of `tile` output elements along an axis of n_out voxels x xc elements: taps() itself, tile by tile
// (the span's width changes with the tile's phase, so neither the end tiles nor a bound from the scale give the exact figure that
// decides the launch form; n_out / 4 evaluations at most, microseconds for a scan).
static int max_span(int n_out, int xc, int tile, float scale, int n_in, bool ac) {
    const long long ne = (long long)n_out * xc;
    int widest = 1;
    for (long long e0 = 0; e0 < ne; e0 += tile) {
        const int first = (int)(e0 / xc), last = (int)((std::min(e0 + (long long)tile, ne) - 1) / xc);
        widest = std::max(widest, taps(last, scale, n_in, ac).i1 - taps(first, scale, n_in, ac).i0 + 1);
    }
    return widest;
}

// Fills the scales and the tile grid; returns false when the grid does not fit a launch, or a lane's 32-bit tap offsets behind its
// brick's first voxel do not reach far enough.  `stage`: every tile's source brick fits the LDS brick (its offsets then span a few planes
// only; the direct gathers index the whole volume with them).
static bool plan_bricks(VRArgs& a, int xc, bool& stage, long long& blocks) {
    const bool ac = a.align != 0;
    a.sd = axis_scale(a.ID, a.RD, a.align); a.sh = axis_scale(a.IH, a.RH, a.align); a.sw = axis_scale(a.IW, a.RW, a.align);
    const long long tx = ((long long)a.RW * xc + VR_TX - 1) / VR_TX, ty = (a.RH + VR_TY - 1) / VR_TY, tz = (a.RD + VR_TZ - 1) / VR_TZ;
    blocks = tx * ty * tz;
    if (tx > 0x7fffffffLL || blocks > 0x7fffffffLL) return false;
    a.tiles_x = (int)tx; a.tiles_y = (int)ty;
    const long long nx = (long long)max_span(a.RW, xc, VR_TX, a.sw, a.IW, ac) * xc;
    const long long ny = max_span(a.RH, 1, VR_TY, a.sh, a.IH, ac), nz = max_span(a.RD, 1, VR_TZ, a.sd, a.ID, ac);
    stage = nx * ny * nz <= VR_BRICK;
    return (stage ? nz : (long long)a.ID) * a.sZ <= 0xffffffffLL;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_volume_resize_trilinear(const void* volume, int in_dtype, int D, int H, int W, int C, int RD, int RH, int RW, int align_corners,
                                           int out_dtype, void* out, ptb_stream_t stream) {
    if (!volume || !out || D < 1 || H < 1 || W < 1 || C < 1 || RD < 1 || RH < 1 || RW < 1) return PTB_EINVAL;
    if (in_dtype < PTB_F32 || in_dtype > PTB_U16 || out_dtype < PTB_F32 || out_dtype > PTB_BF16) return PTB_EINVAL;
    if (C > MAX_VRESIZE_C) return PTB_EUNSUPPORTED;
    if ((long long)W * C > 0x7fffffffLL || (long long)RW * C > 0x7fffffffLL) return PTB_EUNSUPPORTED;   // a row is indexed with 32 bits
    VRArgs a{};
    a.vol = volume; a.out = out;
    a.sY = (long long)W * C; a.sZ = (long long)H * W * C;
    a.C = C; a.ID = D; a.IH = H; a.IW = W; a.RD = RD; a.RH = RH; a.RW = RW;
    a.align = align_corners ? 1 : 0;
    bool stage;
    long long blocks;
    if (!plan_bricks(a, C, stage, blocks)) return PTB_EUNSUPPORTED;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
    with_value<PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16, PTB_U16>(in_dtype, [&](auto in) {
        with_value<PTB_F32, PTB_F16, PTB_BF16>(out_dtype, [&](auto o) { with_bool(stage, [&](auto st) {
            hipLaunchKernelGGL((volume_resize_kernel<in(), o(), st()>), grid, block, 0, s, a); }); }); });
    return check_launch();
}
