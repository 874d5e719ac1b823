// Confusion matrix of two label maps, or of logits and a label map, on the device: cm[t, p] = number of positions with target == t and
// pred == p, int64, ADDED to what the caller's matrix holds.  (The reference has no metrics module; this is the scoring step behind
// merge_crop(argmax=True) and behind a validation batch.)
//
// LAYOUT.  A lane owns a run of P consecutive positions per trip: 16 bytes of the narrower input (labels), 4 fp32 / 8 half positions
// (logits: the C planes are walked with a running best per owned position -- first maximum wins, NaN counts as the maximum, the rule of
// ptb_merge_crop.hip; C == 1: logit > threshold).  A chunk is what the 256 lanes of a workgroup own in one trip; workgroups take the
// chunks of their group (a sample, or all samples pooled) grid-stride, gridDim.x sized from the CU count and never from n.
// WIDE / PEELED.  One kernel holds both bodies and picks per chunk, uniformly for the workgroup: a chunk that lies whole inside its sample
// and whose sample bases are 16-byte aligned is read with 16-byte loads; tails and samples at odd bases (b * n_per_sample * elem_bytes is
// rarely a multiple of 16) are read element by element with the same ownership.  Every input byte is read once per row block.
// COUNTING, FLUSH: ptb_confusion_device.h.  No workspace: the flush is 64-bit integer vector atomics on the result, exact and
// independent of arrival order, at most rows * K per workgroup and only for non-zero cells.
#include <algorithm>

#include "ptb_confusion_device.h"
#include "ptb_dispatch.h"

namespace ptb {

struct ConfLabelsArgs {
    ConfMatrix m;
    const void* pred;
    const void* target;
    long long n;            // positions per sample
    long long chunks;       // per sample
};

struct ConfLogitsArgs {
    ConfMatrix m;
    const void* logits;     // [N, C, S]
    const void* target;     // [N, S]
    long long S, chunks;    // chunks per sample
    long long spg;          // samples per group: 1 (per sample) or N (pooled)
    int C;
    int planes_aligned;     // logits base and S * elem_bytes are multiples of 16: every plane starts on a 16-byte boundary
    float threshold;
};

template <class TP, class TT>
__global__ __launch_bounds__(CONF_THREADS) void confusion_labels_kernel(const ConfLabelsArgs a) {
    constexpr int NB = sizeof(TP) < sizeof(TT) ? sizeof(TP) : sizeof(TT);
    constexpr int P = 16 / NB;
    constexpr long long CH = (long long)CONF_THREADS * P;
    using WP = conf_wide_t<TP>;
    using WT = conf_wide_t<TT>;
    ConfLane s;
    const ConfBlock b = conf_begin(a.m, s);
    const long long g = (long long)a.m.g0 + blockIdx.z;
    const TP* pred = reinterpret_cast<const TP*>(a.pred) + g * a.n;
    const TT* target = reinterpret_cast<const TT*>(a.target) + g * a.n;
    const bool aligned = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) & 15u) == 0;
    const WT ignore = (WT)a.m.ignore;
    const bool has_ignore = a.m.has_ignore != 0 && (long long)ignore == a.m.ignore;      // a value outside the type occurs nowhere

#pragma unroll 1
    for (long long c = blockIdx.x; c < a.chunks; c += gridDim.x) {
        const long long i0 = c * CH + (long long)threadIdx.x * P;
        if (aligned && (c + 1) * CH <= a.n) {
            TP pv[P];
            TT tv[P];
            __builtin_memcpy(pv, __builtin_assume_aligned(pred + i0, 16), sizeof(pv));
            __builtin_memcpy(tv, __builtin_assume_aligned(target + i0, 16), sizeof(tv));
#pragma unroll
            for (int j = 0; j < P; ++j) conf_push<WT, WP>(s, b, (WT)tv[j], (WP)pv[j], has_ignore, ignore);
        } else {
#pragma unroll 1
            for (int j = 0; j < P; ++j)
                if (i0 + j < a.n) conf_push<WT, WP>(s, b, (WT)target[i0 + j], (WP)pred[i0 + j], has_ignore, ignore);
        }
    }
    conf_finish(a.m, b, s);
}

// LD: 1 = fp32, 2 = fp16, 3 = bf16 (ptb_dispatch.h); the half types travel as their 16 bits
template <int LD>
__device__ __forceinline__ float conf_from_bits(unsigned short h) {
    if constexpr (LD == 2) return (float)__builtin_bit_cast(_Float16, h);
    else return __uint_as_float((unsigned)h << 16);
}

template <int LD>
__device__ __forceinline__ float conf_widen(const void* p, long long i) {
    if constexpr (LD == 1) return reinterpret_cast<const float*>(p)[i];
    else return conf_from_bits<LD>(reinterpret_cast<const unsigned short*>(p)[i]);
}

template <int LD, class TT>
__global__ __launch_bounds__(CONF_THREADS) void confusion_logits_kernel(const ConfLogitsArgs a) {
    constexpr int P = LD == 1 ? 4 : 8;
    constexpr int EB = LD == 1 ? 4 : 2;
    constexpr long long CH = (long long)CONF_THREADS * P;
    constexpr int TA = P * (int)sizeof(TT) < 16 ? P * (int)sizeof(TT) : 16;      // alignment of a lane's target run
    using WT = conf_wide_t<TT>;
    ConfLane s;
    const ConfBlock b = conf_begin(a.m, s);
    const long long g = (long long)a.m.g0 + blockIdx.z;
    const WT ignore = (WT)a.m.ignore;
    const bool has_ignore = a.m.has_ignore != 0 && (long long)ignore == a.m.ignore;
    const long long items = a.spg * a.chunks;
    const int C = a.C;

#pragma unroll 1
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long sn = it / a.chunks, c = it - sn * a.chunks, n = g * a.spg + sn;
        const char* lg = reinterpret_cast<const char*>(a.logits) + n * C * a.S * EB;
        const TT* tg = reinterpret_cast<const TT*>(a.target) + n * a.S;
        const long long s0 = c * CH + (long long)threadIdx.x * P;
        const bool wide = a.planes_aligned != 0 && (reinterpret_cast<uintptr_t>(tg) & (TA - 1)) == 0 && (c + 1) * CH <= a.S;
        float best[P];
        int arg[P];
        TT tv[P];
#pragma unroll
        for (int j = 0; j < P; ++j) { best[j] = 0.f; arg[j] = 0; tv[j] = (TT)0; }
        if (wide) {
#pragma unroll 2
            for (int ch = 0; ch < C; ++ch) {
                const char* plane = lg + ((long long)ch * a.S + s0) * EB;
                float v[P];
                if constexpr (LD == 1) {
                    __builtin_memcpy(v, __builtin_assume_aligned(plane, 16), 16);
                } else {
                    unsigned short h[P];
                    __builtin_memcpy(h, __builtin_assume_aligned(plane, 16), 16);
#pragma unroll
                    for (int j = 0; j < P; ++j) v[j] = conf_from_bits<LD>(h[j]);
                }
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const bool take = ch == 0 || v[j] > best[j] || (v[j] != v[j] && best[j] == best[j]);
                    best[j] = take ? v[j] : best[j];
                    arg[j] = take ? ch : arg[j];
                }
            }
            __builtin_memcpy(tv, __builtin_assume_aligned(tg + s0, TA), sizeof(tv));
        } else {
#pragma unroll 1
            for (int ch = 0; ch < C; ++ch) {
                const char* plane = lg + (long long)ch * a.S * EB;
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    if (s0 + j < a.S) {
                        const float v = conf_widen<LD>(plane, s0 + j);
                        const bool take = ch == 0 || v > best[j] || (v != v && best[j] == best[j]);
                        best[j] = take ? v : best[j];
                        arg[j] = take ? ch : arg[j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < P; ++j)
                if (s0 + j < a.S) tv[j] = tg[s0 + j];
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = C == 1 ? (int)(best[j] > a.threshold) : arg[j];                   // (NaN > threshold is false: 0)
            if (wide || s0 + j < a.S) conf_push<WT, int>(s, b, (WT)tv[j], p, has_ignore, ignore);
        }
    }
    conf_finish(a.m, b, s);
}

// ---------------------------------------------------------------------------------------------------------- host side
struct ConfPlan {
    int rows, row_blocks, lds_bytes;
};

static int conf_plan(int K, ConfPlan& p) {
    if (K < 1) return PTB_EINVAL;
    if (K > CONF_MAX_K) return PTB_EUNSUPPORTED;
    p.rows = std::min(K, CONF_HIST_MAX / K);
    p.row_blocks = (K + p.rows - 1) / p.rows;
    p.lds_bytes = p.rows * K * 4;
    return PTB_OK;
}

static int conf_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) {
            (void)hipGetLastError();
            v = 256;
        }
        cus = v;
    }
    return cus;
}

// gridDim.x for `items` chunks of `ch` positions per group: towards as many workgroups as the CUs hold at this LDS size over all groups
// and row blocks of the launch, and at least so many that no workgroup visits more than CONF_MAX_POS_PER_WG (+ one chunk) positions
static int conf_grid_x(long long items, long long ch, long long groups, const ConfPlan& p, unsigned& gx) {
    const int per_cu = std::max(1, std::min(8, 160 * 1024 / p.lds_bytes));
    const long long want = std::max<long long>(1, (long long)conf_cus() * per_cu / (groups * p.row_blocks));
    const long long need = (items + CONF_MAX_POS_PER_WG / ch - 1) / (CONF_MAX_POS_PER_WG / ch);
    const long long x = std::min(items, std::max(want, need));
    if (x > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    gx = (unsigned)x;
    return PTB_OK;
}

constexpr long long CONF_MAX_ELEMS = 1LL << 60;
constexpr int CONF_MAX_Z = 65535;

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_confusion_plan(int K, int* row_blocks, int* lds_bytes) {
    ConfPlan p;
    if (int rc = conf_plan(K, p)) return rc;
    if (row_blocks) *row_blocks = p.row_blocks;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return PTB_OK;
}

extern "C" int ptb_confusion_labels(const void* pred, int pred_elem_bytes, const void* target, int target_elem_bytes, int64_t B, int64_t n_per_sample,
                                    int K, int has_ignore, int64_t ignore_index, int64_t* out, int64_t* invalid, ptb_stream_t stream) {
    if (!pred || !target || !out || !invalid || bad_elem_bytes(pred_elem_bytes) || bad_elem_bytes(target_elem_bytes) || B < 1 || n_per_sample < 1) return PTB_EINVAL;
    if (B > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    ConfPlan p;
    if (int rc = conf_plan(K, p)) return rc;
    if (n_per_sample > CONF_MAX_ELEMS / B) return PTB_EUNSUPPORTED;
    const int P = 16 / std::min(pred_elem_bytes, target_elem_bytes);
    const long long ch = (long long)CONF_THREADS * P;
    ConfLabelsArgs a{};
    a.m.out = reinterpret_cast<long long*>(out); a.m.invalid = reinterpret_cast<long long*>(invalid);
    a.m.ignore = ignore_index; a.m.has_ignore = has_ignore != 0; a.m.K = K; a.m.rows = p.rows;
    a.pred = pred; a.target = target; a.n = n_per_sample; a.chunks = (n_per_sample + ch - 1) / ch;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t g0 = 0; g0 < B; g0 += CONF_MAX_Z) {
        const long long groups = std::min<int64_t>(CONF_MAX_Z, B - g0);
        unsigned gx;
        if (int rc = conf_grid_x(a.chunks, ch, groups, p, gx)) return rc;
        a.m.g0 = (int)g0;
        const dim3 grid(gx, (unsigned)p.row_blocks, (unsigned)groups);
        with_value<1, 2, 4, 8>(pred_elem_bytes, [&](auto pe) {
            with_value<1, 2, 4, 8>(target_elem_bytes, [&](auto te) {
                hipLaunchKernelGGL((confusion_labels_kernel<label_t<pe()>, label_t<te()>>), grid, dim3(CONF_THREADS), (size_t)p.lds_bytes, s, a);
            });
        });
        if (int rc = check_launch()) return rc;
    }
    return PTB_OK;
}

extern "C" int ptb_confusion_logits(const void* logits, int dtype, int64_t N, int C, int64_t S, float threshold, const void* target, int target_elem_bytes,
                                    int per_sample, int has_ignore, int64_t ignore_index, int64_t* out, int64_t* invalid, ptb_stream_t stream) {
    if (!logits || !target || !out || !invalid || bad_elem_bytes(target_elem_bytes) || N < 1 || C < 1 || S < 1) return PTB_EINVAL;
    if (dtype != PTB_F32 && dtype != PTB_F16 && dtype != PTB_BF16) return PTB_EINVAL;
    if (C > CONF_MAX_K) return PTB_EUNSUPPORTED;
    ConfPlan p;
    if (int rc = conf_plan(C == 1 ? 2 : C, p)) return rc;
    if (S > CONF_MAX_ELEMS / N / C || N > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    const int eb = dtype == PTB_F32 ? 4 : 2, P = 16 / eb;
    const long long ch = (long long)CONF_THREADS * P;
    ConfLogitsArgs a{};
    a.m.out = reinterpret_cast<long long*>(out); a.m.invalid = reinterpret_cast<long long*>(invalid);
    a.m.ignore = ignore_index; a.m.has_ignore = has_ignore != 0; a.m.K = C == 1 ? 2 : C; a.m.rows = p.rows;
    a.logits = logits; a.target = target; a.S = S; a.chunks = (S + ch - 1) / ch; a.C = C; a.threshold = threshold;
    a.spg = per_sample ? 1 : N;
    a.planes_aligned = aligned16(logits) && (S * eb) % 16 == 0;
    const int64_t G = per_sample ? N : 1;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t g0 = 0; g0 < G; g0 += CONF_MAX_Z) {
        const long long groups = std::min<int64_t>(CONF_MAX_Z, G - g0);
        unsigned gx;
        if (int rc = conf_grid_x(a.spg * a.chunks, ch, groups, p, gx)) return rc;
        a.m.g0 = (int)g0;
        const dim3 grid(gx, (unsigned)p.row_blocks, (unsigned)groups);
        with_src_dtype(dtype, [&](auto ld) {
            with_value<1, 2, 4, 8>(target_elem_bytes, [&](auto te) {
                hipLaunchKernelGGL((confusion_logits_kernel<ld(), label_t<te()>>), grid, dim3(CONF_THREADS), (size_t)p.lds_bytes, s, a);
            });
        });
        if (int rc = check_launch()) return rc;
    }
    return PTB_OK;
}
