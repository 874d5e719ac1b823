// ptb_edges.hip -- the split end of the tiled-inference loop, on the device:
//
//   * ptb_split_tiles (and its uint8 / fp32 form ptb_split_tiles_u8): ImageSlicer.split (tiles.py:177-204; any of the five
//     OpenCV borders) + image_to_tensor (utils/torch_utils.py:204-231, HWC -> CHW) + .float() [+ per-channel affine]
//     [+ *_image_augment, tta.py:257-284,319-341,385-422,470-484] [+ .to(half | bf16)] from a device-resident uint8 / uint16 /
//     int16 HWC image straight into the chunk-major batch [V*B, C, th, tw] the model consumes.
//     The reference pads the whole image on the host, materialises 361 tile views, converts each to CHW, stacks, casts
//     and uploads 1.14 GB of fp32; here 75 MB of uint8 go up once and each output element is written exactly once.
//
// The other end, merge + crop, is in ptb_merge_crop.hip.  The split is an HBM-bound streaming kernel (no MFMA), write-bound (V*4
// output bytes per input byte); it reuses the augment scatter of the view kernels: one 64 x CH pixel chunk per workgroup, 16 B
// stores per lane, transposing views through the XOR-swizzled LDS tile.
#include "ptb_dispatch.h"
#include "ptb_view_device.h"

namespace ptb {

constexpr int MAX_SPLIT_C = 16;

struct SplitArgs {
    const void* img;     // [IH, IW, IC] of IN (PTB_U8 | PTB_U16 | PTB_I16), contiguous
    int IH, IW, IC;
    int b0;              // batch index of the first tile of this launch group
    int border;          // PTB_BORDER_*: how pixels outside the image are found (workgroup-uniform)
    float pad;           // PTB_BORDER_CONSTANT: border value (already a value of the image's type, as float)
    int affine;          // 0: out = float(in); 1: out = float(in) * scale[c] + bias[c] (two roundings, like torch)
    float scale[MAX_SPLIT_C], bias[MAX_SPLIT_C];
    int tx[MAX_GROUP], ty[MAX_GROUP];  // tile origins in image coordinates; tiles may hang over any border
};

// Index map of np.pad for one axis of n pixels (i may lie any distance outside [0, n)): what ImageSlicer.split's _pad2d reads.
__device__ __forceinline__ int border_index(int i, int n, int border) {
    if (border == PTB_BORDER_REPLICATE) return min(max(i, 0), n - 1);                         // "edge"
    if (border == PTB_BORDER_WRAP) { const int j = i % n; return j < 0 ? j + n : j; }         // "wrap"
    if (border == PTB_BORDER_REFLECT) {                                                      // "symmetric"
        int j = i % (2 * n);
        j = j < 0 ? j + 2 * n : j;
        return j < n ? j : 2 * n - 1 - j;
    }
    if (n == 1) return 0;                                                                    // "reflect" (REFLECT_101)
    const int p = 2 * (n - 1);
    int j = i % p;
    j = j < 0 ? j + p : j;
    return j < n ? j : p - j;
}

// pixel (gy, gx), channel c of the image widened to fp32 (exact for 8- and 16-bit integers); (gy, gx) inside the image
template <int IN>
__device__ __forceinline__ float split_load(const SplitArgs& g, int gy, int gx, int c) {
    return widen<IN>(g.img, ((long long)gy * g.IW + gx) * g.IC + c);
}

// pixel (gy, gx) of the padded image [+ affine].  `inside` (uniform): the caller knows the pixel lies in the image, no test, no remap.
template <int IN>
__device__ __forceinline__ float split_pixel(const SplitArgs& g, int gy, int gx, int c, bool inside) {
    float f;
    if (inside || (gy >= 0 && gy < g.IH && gx >= 0 && gx < g.IW)) f = split_load<IN>(g, gy, gx, c);
    else if (g.border == PTB_BORDER_CONSTANT) f = g.pad;
    else f = split_load<IN>(g, border_index(gy, g.IH, g.border), border_index(gx, g.IW, g.border), c);
    if (g.affine) f = __fadd_rn(__fmul_rn(f, g.scale[c]), g.bias[c]);
    return f;
}

template <int CH, int IN, int OUT>
__global__ __launch_bounds__(CH * 16) void edge_split_kernel(const ViewArgs a, const SplitArgs g, int B) {
    __shared__ __attribute__((aligned(16))) float st[CW * CH];
    const int tid = threadIdx.x;
    const int cpt = a.chunks_x * a.chunks_y;
    int bid = blockIdx.x;
    const int chunk = bid % cpt;
    bid /= cpt;
    const int c = bid % a.C;
    const int lb = bid / a.C;  // tile within this launch group
    const int x0 = (chunk % a.chunks_x) * CW, y0 = (chunk / a.chunks_x) * CH;
    const int cw = min(CW, a.W - x0), ch = min(CH, a.H - y0);
    const int sy = g.ty[lb] + y0, sx = g.tx[lb] + x0;  // the chunk's source rectangle: [sy, sy + ch) x [sx, sx + cw)
    const bool inside = sy >= 0 && sy + ch <= g.IH && sx >= 0 && sx + cw <= g.IW;
    const int q = tid & 15, r = tid >> 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < ch && 4 * q < cw) {
        const int gy = sy + r, gx = sx + 4 * q;
        v.x = split_pixel<IN>(g, gy, gx, c, inside);
        v.y = split_pixel<IN>(g, gy, gx + 1, c, inside);
        v.z = split_pixel<IN>(g, gy, gx + 2, c, inside);
        v.w = split_pixel<IN>(g, gy, gx + 3, c, inside);
    }
    scatter_chunk<CH, false, OUT>(a, B, g.b0 + lb, c, x0, y0, cw, ch, v, st, tid);
}

// any tile shape: one output element per thread (grid-stride over this group's V * n * C * th * tw elements)
template <int IN, int OUT>
__global__ __launch_bounds__(256) void edge_split_scalar_kernel(const ViewArgs a, const SplitArgs g, int B, int n) {
    const long long plane = (long long)a.H * a.W;
    const long long per_view = (long long)n * a.C * plane;
    const long long total = per_view * a.nviews;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int k = (int)(t / per_view);
        long long rem = t - (long long)k * per_view;
        const int lb = (int)(rem / (a.C * plane));
        rem -= (long long)lb * a.C * plane;
        const int c = (int)(rem / plane);
        const long long px = rem - (long long)c * plane;
        const int i = (int)(px / a.W), j = (int)(px - (long long)i * a.W);
        const int code = (a.codes >> (3 * k)) & 7;
        int R, Cc;  // source (tile-local) pixel of output (i, j) of view k
        if (code & 1) { R = (code & 2) ? a.H - 1 - j : j; Cc = (code & 4) ? a.W - 1 - i : i; }
        else { R = (code & 2) ? a.H - 1 - i : i; Cc = (code & 4) ? a.W - 1 - j : j; }
        const float f = split_pixel<IN>(g, g.ty[lb] + R, g.tx[lb] + Cc, c, false);
        const long long o = (((long long)k * B + g.b0 + lb) * a.C + c) * plane + px;
        if constexpr (OUT == PTB_F32) a.dst[o] = f;
        else reinterpret_cast<unsigned short*>(a.dst)[o] = half_bits<OUT>(f);
    }
}

// one launch per group of MAX_GROUP tiles: the LDS-scatter kernel (CH rows per chunk, ptb_set_tunable key 0) or, for any other
// shape / ptb_set_tunable(1, 1), the scalar kernel
static int launch_split_tiles(int in_dtype, int out_dtype, ViewArgs& a, SplitArgs& g, const int64_t* xs, const int64_t* ys, int B, int V, bool fast,
                              hipStream_t s) {
    const int ch = g_chunk_rows;
    for (int b0 = 0; b0 < B; b0 += MAX_GROUP) {
        const int n = B - b0 < MAX_GROUP ? B - b0 : MAX_GROUP;
        g.b0 = b0;
        for (int t = 0; t < n; ++t) { g.tx[t] = (int)xs[b0 + t]; g.ty[t] = (int)ys[b0 + t]; }
        if (fast) {
            const long long blocks = (long long)n * g.IC * a.chunks_x * a.chunks_y;
            if (blocks > 0x7fffffffLL) return PTB_EUNSUPPORTED;
            with_value<64, 32, 16>(ch, [&](auto chv) { with_value<PTB_U8, PTB_U16, PTB_I16>(in_dtype, [&](auto in) {
                with_value<PTB_F32, PTB_F16, PTB_BF16>(out_dtype, [&](auto out) {
                    hipLaunchKernelGGL((edge_split_kernel<chv(), in(), out()>), dim3((unsigned)blocks), dim3(chv() * 16), 0, s, a, g, B);
                }); }); });
        } else {
            const long long total = (long long)V * n * g.IC * a.H * a.W;
            const long long want = (total + 255) / 256;
            with_value<PTB_U8, PTB_U16, PTB_I16>(in_dtype, [&](auto in) { with_value<PTB_F32, PTB_F16, PTB_BF16>(out_dtype, [&](auto out) {
                hipLaunchKernelGGL((edge_split_scalar_kernel<in(), out()>), dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, s, a, g, B, n);
            }); });
        }
        if (int rc = check_launch()) return rc;
    }
    return PTB_OK;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_split_tiles(const void* image, int in_dtype, int IH, int IW, int IC, const int64_t* xs, const int64_t* ys, int B, int th,
                               int tw, int V, const int* views, const float* scale, const float* bias, int border, float pad_value,
                               int out_dtype, void* out, ptb_stream_t stream) {
    if (!image || !out || !xs || !ys || IH < 1 || IW < 1 || IC < 1 || B < 0 || th < 1 || tw < 1) return PTB_EINVAL;
    if (in_dtype == PTB_F32 || in_dtype == PTB_F16 || in_dtype == PTB_BF16) return PTB_EUNSUPPORTED;   // float images: not a split source
    if (in_dtype != PTB_U8 && in_dtype != PTB_U16 && in_dtype != PTB_I16) return PTB_EINVAL;
    if (out_dtype != PTB_F32 && out_dtype != PTB_F16 && out_dtype != PTB_BF16) return PTB_EINVAL;
    if (border == 5 || border == 16) return PTB_EUNSUPPORTED;   // cv2.BORDER_TRANSPARENT / BORDER_ISOLATED: refused by split too
    if (border < PTB_BORDER_CONSTANT || border > PTB_BORDER_REFLECT_101) return PTB_EINVAL;
    if (IC > MAX_SPLIT_C) return PTB_EUNSUPPORTED;
    if (border == PTB_BORDER_CONSTANT) {   // a value of the image's type
        const float lo = in_dtype == PTB_U8 ? 0.f : (in_dtype == PTB_U16 ? 0.f : -32768.f);
        const float hi = in_dtype == PTB_U8 ? 255.f : (in_dtype == PTB_U16 ? 65535.f : 32767.f);
        if (!(pad_value >= lo && pad_value <= hi) || pad_value != truncf(pad_value)) return PTB_EINVAL;
    }
    if ((scale == nullptr) != (bias == nullptr)) return PTB_EINVAL;
    if (V < 1 || V > 8 || !views) return PTB_EINVAL;
    int codes = 0, nt = 0;
    for (int k = 0; k < V; ++k) {
        if (views[k] < 0 || views[k] > 7) return PTB_EINVAL;
        codes |= views[k] << (3 * k);
        nt += views[k] & 1;
    }
    if (nt && th != tw) return PTB_EINVAL;
    for (int b = 0; b < B; ++b) {  // a tile may hang over the border but must be addressable with 32-bit coordinates
        if (xs[b] < -(1 << 30) || xs[b] > (1 << 30) || ys[b] < -(1 << 30) || ys[b] > (1 << 30)) return PTB_EBOUNDS;
    }
    if (B == 0) return PTB_OK;
    ViewArgs a{};
    a.dst = static_cast<float*>(out);   // (element type out_dtype: the kernels' stores convert)
    a.H = th; a.W = tw; a.C = IC;
    a.nviews = V;
    a.codes = codes;
    a.scale = 1.0f;
    a.chunks_x = (tw + CW - 1) / CW;
    a.chunks_y = (th + g_chunk_rows - 1) / g_chunk_rows;
    SplitArgs g{};
    g.img = image; g.IH = IH; g.IW = IW; g.IC = IC;
    g.border = border;
    g.pad = pad_value;
    g.affine = scale ? 1 : 0;
    for (int c = 0; c < IC; ++c) { g.scale[c] = scale ? scale[c] : 1.0f; g.bias[c] = bias ? bias[c] : 0.0f; }
    const bool fast = !g_force_scalar && tw % 4 == 0 && (nt == 0 || th % 4 == 0) && aligned16(out);
    hipStream_t s = (hipStream_t)stream;
    return launch_split_tiles(in_dtype, out_dtype, a, g, xs, ys, B, V, fast, s);
}

// The uint8 / constant border / fp32 contract of the first device split, kept as it was (the same checks in the same order).
extern "C" int ptb_split_tiles_u8(const uint8_t* image, int IH, int IW, int IC, const int64_t* xs, const int64_t* ys, int B,
                                  int th, int tw, int V, const int* views, const float* scale, const float* bias, int pad_value,
                                  float* out, ptb_stream_t stream) {
    if (!image || !out || !xs || !ys || IH < 1 || IW < 1 || IC < 1 || B < 0 || th < 1 || tw < 1) return PTB_EINVAL;
    if (IC > MAX_SPLIT_C) return PTB_EUNSUPPORTED;
    if (pad_value < 0 || pad_value > 255) return PTB_EINVAL;
    return ptb_split_tiles(image, PTB_U8, IH, IW, IC, xs, ys, B, th, tw, V, views, scale, bias, PTB_BORDER_CONSTANT, (float)pad_value,
                           PTB_F32, out, stream);
}
