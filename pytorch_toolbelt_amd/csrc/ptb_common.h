// Internal helpers shared by the libptb_hip translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/ptb_hip.h"

namespace ptb {

// thread-local text of the last failing HIP call (ptb_last_hip_error)
void set_hip_error(hipError_t e);
void set_error_text(const char* text);   // the text ptb_last_hip_error() returns for PTB_ELAUNCH (non-HIP failures: RCCL)

inline int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_hip_error(e);
        return PTB_ELAUNCH;
    }
    return PTB_OK;
}

// Results that are written once and not read again by the same launch (merged maps, de-augmented tiles, augmented batches,
// gradients): non-temporal 16-byte stores, so that hundreds of MB of output do not displace the lines the kernel still reads from
// L2 / Infinity Cache.  -DPTB_NT_OUT=0 builds the plain-store variant for A/B runs (tools/build_variant.sh).
#ifndef PTB_NT_OUT
#define PTB_NT_OUT 1
#endif
__device__ __forceinline__ void out_store4(float* p, const float4 v) {
#if PTB_NT_OUT
    typedef float ptb_v4f __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(ptb_v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<ptb_v4f*>(p));
#else
    *reinterpret_cast<float4*>(p) = v;
#endif
}

// Index of the wave inside its workgroup as a SCALAR: every lane of a wave computes the same threadIdx.x >> 6, but only through
// readfirstlane does the compiler know it, and everything derived from it (grid-stride group index, image / plane offsets, base
// addresses) then runs on the scalar unit and the loads take an SGPR base -- on the loss kernels that was 7 of 25 vector
// instructions per element.
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline long long up16(long long v) { return (v + 15) & ~15LL; }

// label maps: the element sizes a call accepts, the integer type of a size, and whether that type holds a value
inline bool bad_elem_bytes(int eb) { return eb != 1 && eb != 2 && eb != 4 && eb != 8; }
template <int EB>
using label_t = std::conditional_t<EB == 1, unsigned char, std::conditional_t<EB == 2, short, std::conditional_t<EB == 4, int, long long>>>;
inline bool holds(int elem_bytes, long long v) {
    switch (elem_bytes) {
        case 1: return v >= 0 && v <= 255;
        case 2: return v >= -32768 && v <= 32767;
        case 4: return v >= -2147483648LL && v <= 2147483647LL;
        default: return true;
    }
}

// the shape of a call over [B] entries of D x H x W positions, all indexed in 32 bits: PTB_EINVAL for what is no shape,
// PTB_EUNSUPPORTED above the limit
constexpr long long MAX_POS = 0x7fffffffLL - 1;
inline int check_shape(int dims, long long B, long long D, long long H, long long W) {
    if ((dims != 2 && dims != 3) || B < 1 || D < 1 || H < 1 || W < 1 || (dims == 2 && D != 1)) return PTB_EINVAL;
    if (D > MAX_POS || H > MAX_POS || W > MAX_POS || H * W > MAX_POS || D * H * W > MAX_POS || B > MAX_POS / (D * H * W)) return PTB_EUNSUPPORTED;
    return PTB_OK;
}

// tunables: ptb_set_tunable(key, value) -- the key, the values it takes, what it selects
extern int g_chunk_rows;         //  0: 16 | 32 | 64, chunk rows of the view / accumulate kernels
extern int g_force_scalar;       //  1: 0 | 1, element-wise kernels instead of the 16-byte ones
extern int g_ms_tiled;           //  3: 0 | 1, LDS-staged multiscale kernel
extern int g_loss_grid_cap;      //  4: >= 0, workgroups per loss-kernel launch (0: the per-kernel default)
extern int g_ms_tile_rows;       //  6: 16 | 32 | 64, output tile height of the fused multiscale kernel
extern int g_smf_bwd_stash;      //  7: 0 | 2 | 4, softmax focal backward with the per-class terms kept in registers, pixels per lane
extern int g_ms_strip;           //  9: 0 | 1..64, XCD-aware tile order of the fused multiscale kernel, strip width in tile columns
extern int g_band_rows;          // 11: 32 | 64, rows per work item of band plans created from now on
extern int g_ms_tile_w;          // 15: 64 | 128, output tile width of the fused multiscale kernel
extern int g_nt_grad_stores;     // 16: 0 | 1, non-temporal gradient stores in the fused loss backward
extern int g_rs_xcd_map;         // 17: 0 | 1 (bit 0 of the value), XCD-contiguous tile order in the Lovasz radix scatter
extern int g_rank_finish_fused;  // 18: 0 | 1, one-launch finish of a rank's image (ShardedTileMerger, deferred bands)
extern int g_lovasz_fused_dot;   // 19: 0 | 1, the binning scatter of the Lovasz training path also evaluates the loss
extern int g_stats_pk;           // 20: 0 | 1, statistics-only / focal-only instances of the packed streaming loss kernel
extern int g_band_half_pf;       // 21: clamped to 0..2, the band plan kernel prefetches the next covering tile (1: half / bf16 sources only, 2: fp32 too)
extern int g_lovasz_rankdot;     // 23: 0 | 1, last level of the key-only Lovasz forward without a scatter
extern int g_band_lds_db;        // 25: 0 | 1, double-buffered LDS tiles in the prefetching band plan instances
extern int g_band_chan_loop;     // 27: 0 | 1, identity-view band launches, one workgroup per item over all channels
extern int g_band_pairs;         // 28: 0 | 1, fp16 / bf16 d4 band launches take the paired items of a group as 64 x 128 blocks (band_pair_kernel)

}  // namespace ptb
