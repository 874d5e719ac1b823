// Distance-map losses (losses/distance_losses.py; the reference has no counterpart): the boundary loss mean(p_k * phi_k) and the
// Hausdorff-DT loss mean((p_k - g_k)^2 * (|phi_pred,k|^alpha + |phi_truth,k|^alpha)), phi the SIGNED distance map of a class's object
// (> 0 outside, < 0 inside) that ptb_edt leaves.  This translation unit holds everything around that transform:
//   1. dl_mask_kernel    one launch writes the uint8 object maps [R, B, K, S] ptb_edt measures in: the truth plane (labels == class_k, or
//                        dense > 0.5) and, for the Hausdorff form, the prediction plane (p_k > 0.5).
//   2. dl_fwd_kernel     one streaming pass over logits, target and map(s); the activation lives in registers.  Every workgroup writes its
//                        fp64 partial sum and its int64 count of elements that are not ignored to ITS OWN slot -- no atomics --
//   3. dl_finish_kernel  and one workgroup per result adds the slots of that result in index order (a lane per run of neighbouring slots,
//                        then lane 0 over the 256 lanes): loss = sum / count, 1 / count for the backward, NaN under a raised label flag.
//   4. dl_bwd_kernel     the gradient for all C channels; the maps are constants.
// Lanes take FOUR NEIGHBOURING POSITIONS: 16-byte loads of logits / maps, 4-byte mask stores where the bases and S % 4 allow (WIDE), a
// peeled instance otherwise.  A softmax sweeps the channels at stride S and keeps them in registers for C <= 16 (buckets 4 / 8 / 16 like
// the other loss kernels; CR = 0: a second sweep instead); sigmoid / identity channels are independent and streamed (CR = -1).
// The grid is a function of the shape alone, a workgroup per 1024 positions of a sample, and the sums are added in a fixed order: a
// second run gives the same bits.  Every loop is bounded by C or K; no workgroup waits for another one.
#include <algorithm>
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_edt_common.h"

namespace ptb {

constexpr int DL_THREADS = 256;
constexpr unsigned DL_SPAN = DL_THREADS * 4;    // positions of a sample per workgroup

struct DlArgs {
    const float* x;             // [B, C, S] logits (probabilities with PTB_PROB_IDENTITY)
    const long long* labels;    // [B, S], or NULL ...
    const float* dense;         // ... and [B, C, S]
    const int* cls;             // [K] the channel of map k; NULL: k itself (K == C)
    const int* slot;            // [C] the map of channel c, -1 for none; NULL: c itself
    const void* phi_t;          // [B, K, S] signed map of the truth: int32 squared, or float32
    const void* phi_p;          // the same of the thresholded prediction (Hausdorff)
    unsigned char* mask_t;      // [B, K, S] object maps to write, or NULL
    unsigned char* mask_p;
    double* psum;               // [B * bps] a slot per workgroup
    long long* pcnt;
    const float* coef;          // [1] or [B]: upstream gradient / count
    float* grad;                // [B, C, S]
    int* flag;
    long long ignore_label;
    float ignore_value, alpha;
    unsigned S, bps;            // positions per sample; workgroups per sample
    int C, K, act, has_ignore, maps_f32, amode, per_sample;
};

// ---------------------------------------------------------------------------------------------------------- four positions
template <bool WIDE, class T>
__device__ __forceinline__ void dl_load4(const T* q, unsigned p0, unsigned S, T (&v)[4], T fill) {
    if constexpr (WIDE) {                                                      // S % 4 == 0 and an aligned base: p0 < S means p0 + 3 < S
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(v, __builtin_assume_aligned(q, A), sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p0 + j < S ? q[j] : fill;
    }
}

template <bool WIDE, class T>
__device__ __forceinline__ void dl_store4(T* q, unsigned p0, unsigned S, const T (&v)[4]) {
    if constexpr (WIDE) {
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(__builtin_assume_aligned(q, A), v, sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < S) q[j] = v[j];
    }
}

// the signed distance a map value stands for; an entry without a boundary (+-inf, +-(2^31 - 1)) counts as 0
__device__ __forceinline__ float dl_signed(int bits, int maps_f32) {
    if (maps_f32) {
        const float f = __int_as_float(bits);
        return fabsf(f) == INFINITY ? 0.0f : f;
    }
    const int m = bits < 0 ? -bits : bits;                                     // (never INT_MIN: the transform leaves |v| <= 2^31 - 1)
    if (m == EDT_INF) return 0.0f;
    const float r = sqrtf((float)m);
    return bits < 0 ? -r : r;
}

// |distance|^alpha.  alpha == 2 on the squared integers takes no root, alpha == 1 only the root; any other alpha is 2^(alpha * log2 d) on the
// hardware's exp2 / log2 (one instruction each; a powf call per element would put a stack frame into the unrolled channel sweep)
__device__ __forceinline__ float dl_power(int bits, const DlArgs& a) {
    if (a.maps_f32) {
        const float f = fabsf(__int_as_float(bits));
        if (f == INFINITY) return 0.0f;
        return a.amode == 2 ? f * f : a.amode == 1 ? f : exp2f(a.alpha * log2f(f));                    // (f == 0: 2^-inf = 0, alpha > 0)
    }
    const int m = bits < 0 ? -bits : bits;
    if (m == EDT_INF) return 0.0f;
    return a.amode == 2 ? (float)m : a.amode == 1 ? sqrtf((float)m) : exp2f(0.5f * a.alpha * log2f((float)m));
}

// ---------------------------------------------------------------------------------------------------------- the channels of four positions
// CR > 0: softmax over C <= CR channels held in registers; CR == 0: softmax with a second sweep over memory; CR == -1: sigmoid / identity.
template <int CR, bool WIDE>
struct DlChannels {
    float xr[CR > 0 ? CR : 1][4];
    float m[4], s[4];

    __device__ __forceinline__ void init(const DlArgs& a, const float* x0, unsigned p0) {
        if constexpr (CR > 0) {
#pragma unroll
            for (int c = 0; c < CR; ++c) {
                if (c < a.C) {
                    dl_load4<WIDE>(x0 + (size_t)c * a.S, p0, a.S, xr[c], 0.0f);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) xr[c][j] = -INFINITY;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float mx = xr[0][j];
#pragma unroll
                for (int c = 1; c < CR; ++c) mx = fmaxf(mx, xr[c][j]);
                float sum = 0.0f;
#pragma unroll
                for (int c = 0; c < CR; ++c) sum += expf(xr[c][j] - mx);
                m[j] = mx;
                s[j] = sum;
            }
        } else if constexpr (CR == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[j] = -INFINITY;
                s[j] = 0.0f;
            }
#pragma unroll 1
            for (int c = 0; c < a.C; ++c) {                                    // the running maximum and the sum with respect to it
                float v[4];
                dl_load4<WIDE>(x0 + (size_t)c * a.S, p0, a.S, v, 0.0f);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (v[j] > m[j]) {
                        s[j] = s[j] * expf(m[j] - v[j]) + 1.0f;
                        m[j] = v[j];
                    } else {
                        s[j] += expf(v[j] - m[j]);
                    }
                }
            }
        }
    }

    __device__ __forceinline__ void prob(const DlArgs& a, const float (&v)[4], float (&p)[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (CR >= 0) p[j] = expf(v[j] - m[j]) / s[j];
            else p[j] = a.act == PTB_PROB_SIGMOID ? 1.0f / (1.0f + expf(-v[j])) : v[j];
        }
    }

    // the held channels one by one, by recursion: every index into xr is a constant whatever the unroller decides about so large a body
    template <int c, class F>
    __device__ __forceinline__ void each_held(const DlArgs& a, F& f) const {
        if constexpr (c < CR) {
            if (c < a.C) {
                float p[4];
                prob(a, xr[c], p);
                f(c, a.slot ? a.slot[c] : c, p);
            }
            each_held<c + 1>(a, f);
        }
    }

    // f(c, k, p[4]) for every channel c of the sample, k its map or -1
    template <class F>
    __device__ __forceinline__ void each(const DlArgs& a, const float* x0, unsigned p0, F&& f) const {
        if constexpr (CR > 0) {
            each_held<0>(a, f);
        } else {
#pragma unroll 1
            for (int c = 0; c < a.C; ++c) {
                float v[4], p[4];
                dl_load4<WIDE>(x0 + (size_t)c * a.S, p0, a.S, v, 0.0f);
                prob(a, v, p);
                f(c, a.slot ? a.slot[c] : c, p);
            }
        }
    }
};

// the labels of four positions: which exist, which are ignored; a label outside [0, C) raises the flag and belongs to no class
template <bool WIDE>
struct DlTarget {
    long long lab[4];
    bool live[4];               // the position exists and its label is not ignored

    __device__ __forceinline__ void init(const DlArgs& a, unsigned b, unsigned p0, bool report) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lab[j] = -1;
            live[j] = WIDE || p0 + j < a.S;
        }
        if (!a.labels) return;
        dl_load4<WIDE>(a.labels + (size_t)b * a.S + p0, p0, a.S, lab, (long long)-1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!live[j]) continue;
            if (a.has_ignore && lab[j] == a.ignore_label) live[j] = false;
            else if (lab[j] < 0 || lab[j] >= a.C) {
                if (report) *a.flag = 1;                                       // (every writer stores the same value)
                lab[j] = -1;
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------- object maps
template <int CR, bool WIDE>
__global__ __launch_bounds__(DL_THREADS) void dl_mask_kernel(const DlArgs a) {
    const unsigned b = blockIdx.x / a.bps;
    const unsigned p0 = ((blockIdx.x - b * a.bps) * DL_THREADS + threadIdx.x) * 4u;
    if (p0 >= a.S) return;
    DlTarget<WIDE> t;
    t.init(a, b, p0, false);
    if (a.mask_t) {
#pragma unroll 1
        for (int k = 0; k < a.K; ++k) {
            const int c = a.cls ? a.cls[k] : k;
            unsigned char o[4];
            if (a.labels) {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = t.live[j] && t.lab[j] == c;
            } else {
                float d[4];
                dl_load4<WIDE>(a.dense + ((size_t)b * a.C + c) * a.S + p0, p0, a.S, d, 0.0f);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = d[j] > 0.5f && !(a.has_ignore && d[j] == a.ignore_value);
            }
            dl_store4<WIDE>(a.mask_t + ((size_t)b * a.K + k) * a.S + p0, p0, a.S, o);
        }
    }
    if (a.mask_p) {
        const float* x0 = a.x + (size_t)b * a.C * a.S + p0;
        DlChannels<CR, WIDE> ch;
        ch.init(a, x0, p0);
        ch.each(a, x0, p0, [&](int, int k, const float (&p)[4]) {
            if (k < 0) return;
            unsigned char o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = p[j] > 0.5f;                    // (a sigmoid's 1 / (1 + exp(-x)) > 0.5 is x > 0)
            dl_store4<WIDE>(a.mask_p + ((size_t)b * a.K + k) * a.S + p0, p0, a.S, o);
        });
    }
}

// ---------------------------------------------------------------------------------------------------------- the loss
// what channel c (map k) of four positions contributes: `use` = the element exists and is not ignored, g its 0 / 1 target
template <bool WIDE>
__device__ __forceinline__ void dl_element(const DlArgs& a, const DlTarget<WIDE>& t, unsigned b, unsigned p0, int c, bool (&use)[4], float (&g)[4]) {
    if (a.labels) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            use[j] = t.live[j];
            g[j] = t.lab[j] == c ? 1.0f : 0.0f;
        }
    } else {
        float d[4];
        dl_load4<WIDE>(a.dense + ((size_t)b * a.C + c) * a.S + p0, p0, a.S, d, 0.0f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            use[j] = t.live[j] && !(a.has_ignore && d[j] == a.ignore_value);
            g[j] = d[j] > 0.5f ? 1.0f : 0.0f;
        }
    }
}

// BOUNDARY: w = phi.  HAUSDORFF: w = |phi_pred|^alpha + |phi_truth|^alpha
template <int KIND, bool WIDE>
__device__ __forceinline__ void dl_weight(const DlArgs& a, unsigned b, unsigned p0, int k, float (&w)[4]) {
    const size_t off = ((size_t)b * a.K + k) * a.S + p0;
    int vt[4];
    dl_load4<WIDE>(reinterpret_cast<const int*>(a.phi_t) + off, p0, a.S, vt, 0);
    if constexpr (KIND == PTB_DLOSS_BOUNDARY) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = dl_signed(vt[j], a.maps_f32);
    } else {
        int vp[4];
        dl_load4<WIDE>(reinterpret_cast<const int*>(a.phi_p) + off, p0, a.S, vp, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = dl_power(vp[j], a) + dl_power(vt[j], a);
    }
}

template <int KIND, int CR, bool WIDE>
__global__ __launch_bounds__(DL_THREADS) void dl_fwd_kernel(const DlArgs a) {
    __shared__ double wsum[DL_THREADS / 64];
    __shared__ long long wcnt[DL_THREADS / 64];
    const unsigned b = blockIdx.x / a.bps;
    const unsigned p0 = ((blockIdx.x - b * a.bps) * DL_THREADS + threadIdx.x) * 4u;
    double sum = 0.0;
    long long cnt = 0;
    if (p0 < a.S) {
        DlTarget<WIDE> t;
        t.init(a, b, p0, true);
        const float* x0 = a.x + (size_t)b * a.C * a.S + p0;
        DlChannels<CR, WIDE> ch;
        ch.init(a, x0, p0);
        ch.each(a, x0, p0, [&](int c, int k, const float (&p)[4]) {
            if (k < 0) return;
            bool use[4];
            float g[4], w[4];
            dl_element<WIDE>(a, t, b, p0, c, use, g);
            dl_weight<KIND, WIDE>(a, b, p0, k, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!use[j]) continue;
                float term;
                if constexpr (KIND == PTB_DLOSS_BOUNDARY) {
                    term = p[j] * w[j];
                } else {
                    const float d = p[j] - g[j];
                    term = d * d * w[j];
                }
                sum += (double)term;
                ++cnt;
            }
        });
    }
    // the workgroup's sum: a fixed tree inside every wave, then the four waves in order
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_down(sum, d);
        cnt += __shfl_down(cnt, d);
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = sum;
        wcnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = wsum[0];
        long long n = wcnt[0];
#pragma unroll
        for (int w = 1; w < DL_THREADS / 64; ++w) {
            r += wsum[w];
            n += wcnt[w];
        }
        a.psum[blockIdx.x] = r;
        a.pcnt[blockIdx.x] = n;
    }
}

struct DlFinishArgs {
    const double* psum;
    const long long* pcnt;
    float* loss;                // [results]
    float* inv_count;           // [results]
    const int* flag;
    unsigned per_result;        // slots of a result
};

__global__ __launch_bounds__(DL_THREADS) void dl_finish_kernel(const DlFinishArgs a) {
    __shared__ double lsum[DL_THREADS];
    __shared__ long long lcnt[DL_THREADS];
    const size_t base = (size_t)blockIdx.x * a.per_result;
    const unsigned run = (a.per_result + DL_THREADS - 1) / DL_THREADS;
    const unsigned lo = min(threadIdx.x * run, a.per_result), hi = min(lo + run, a.per_result);
    double r = 0.0;
    long long n = 0;
#pragma unroll 1
    for (unsigned i = lo; i < hi; ++i) {
        r += a.psum[base + i];
        n += a.pcnt[base + i];
    }
    lsum[threadIdx.x] = r;
    lcnt[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (int i = 1; i < DL_THREADS; ++i) {
            r += lsum[i];
            n += lcnt[i];
        }
        const bool bad = a.flag && *a.flag != 0;                               // a label outside [0, C): never a finite loss
        a.loss[blockIdx.x] = bad ? NAN : (float)(r / (double)n);
        a.inv_count[blockIdx.x] = (float)(1.0 / (double)n);
    }
}

// ---------------------------------------------------------------------------------------------------------- the gradient
// t = coef * phi (boundary) or coef * 2 (p - g) F (Hausdorff) where the element counts, else 0
template <int KIND>
__device__ __forceinline__ float dl_dterm(float coef, float p, float g, float w) {
    if constexpr (KIND == PTB_DLOSS_BOUNDARY) return coef * w;
    else return coef * (2.0f * (p - g) * w);
}

template <int KIND, int CR, bool WIDE>
__global__ __launch_bounds__(DL_THREADS) void dl_bwd_kernel(const DlArgs a) {
    const unsigned b = blockIdx.x / a.bps;
    const unsigned p0 = ((blockIdx.x - b * a.bps) * DL_THREADS + threadIdx.x) * 4u;
    if (p0 >= a.S) return;
    const float coef = a.coef[a.per_sample ? b : 0u];
    DlTarget<WIDE> t;
    t.init(a, b, p0, false);
    const float* x0 = a.x + (size_t)b * a.C * a.S + p0;
    float* g0 = a.grad + (size_t)b * a.C * a.S + p0;
    DlChannels<CR, WIDE> ch;
    ch.init(a, x0, p0);
    auto dterm = [&](int c, int k, const float (&p)[4], float (&d)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = 0.0f;
        if (k < 0) return;
        bool use[4];
        float g[4], w[4];
        dl_element<WIDE>(a, t, b, p0, c, use, g);
        dl_weight<KIND, WIDE>(a, b, p0, k, w);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (use[j]) d[j] = dl_dterm<KIND>(coef, p[j], g[j], w[j]);
    };
    if constexpr (CR >= 0) {                                                   // softmax: grad_c = p_c (t_c - sum_j p_j t_j)
        float dot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        ch.each(a, x0, p0, [&](int c, int k, const float (&p)[4]) {
            if (k < 0) return;
            float d[4];
            dterm(c, k, p, d);
#pragma unroll
            for (int j = 0; j < 4; ++j) dot[j] += p[j] * d[j];
        });
        ch.each(a, x0, p0, [&](int c, int k, const float (&p)[4]) {
            float d[4], r[4];
            dterm(c, k, p, d);                                                 // (its loads hit the lines the sweep above brought in)
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = t.live[j] ? p[j] * (d[j] - dot[j]) : 0.0f;
            dl_store4<WIDE>(g0 + (size_t)c * a.S, p0, a.S, r);
        });
    } else {
        ch.each(a, x0, p0, [&](int c, int k, const float (&p)[4]) {
            float d[4], r[4];
            dterm(c, k, p, d);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = a.act == PTB_PROB_SIGMOID ? p[j] * (1.0f - p[j]) * d[j] : d[j];
            dl_store4<WIDE>(g0 + (size_t)c * a.S, p0, a.S, r);
        });
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// CR of a launch: the register bucket of a softmax, 0 above 16 channels, -1 for independent channels
template <class F>
static void dl_with_channels(int prob, int C, F&& f) {
    if (prob != PTB_PROB_SOFTMAX) f(int_c<-1>{});
    else if (C > 16) f(int_c<0>{});
    else with_at_most<4, 8, 16>(C, f);
}

static bool dl_aligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

static long long dl_blocks_per_sample(long long S) { return (S + DL_SPAN - 1) / DL_SPAN; }

// what every entry point checks of the problem; fills the shape part of the arguments
static int dl_common(const float* logits, bool need_logits, const int64_t* labels, const float* dense, const int* classes, const int* class_table, int B, int C, int K,
                     int64_t S, int prob, DlArgs& a) {
    if ((need_logits && !logits) || (labels != nullptr) == (dense != nullptr)) return PTB_EINVAL;
    if (B < 1 || C < 1 || S < 1 || K < 1 || K > C) return PTB_EINVAL;
    if (prob != PTB_PROB_SOFTMAX && prob != PTB_PROB_SIGMOID && prob != PTB_PROB_IDENTITY) return PTB_EINVAL;
    if ((classes != nullptr) != (class_table != nullptr) || (!classes && K != C)) return PTB_EINVAL;
    if (classes) {
        for (int k = 0; k < K; ++k) {
            if (classes[k] < 0 || classes[k] >= C) return PTB_EINVAL;
            for (int i = 0; i < k; ++i)
                if (classes[i] == classes[k]) return PTB_EINVAL;
        }
    }
    if (S > MAX_POS || (long long)B * dl_blocks_per_sample(S) > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    a.x = logits; a.labels = reinterpret_cast<const long long*>(labels); a.dense = dense;
    a.cls = class_table; a.slot = class_table ? class_table + K : nullptr;
    a.S = (unsigned)S; a.bps = (unsigned)dl_blocks_per_sample(S); a.C = C; a.K = K; a.act = prob;
    return PTB_OK;
}

static bool dl_wide_inputs(const DlArgs& a) {
    return a.S % 4 == 0 && dl_aligned(a.x, 16) && dl_aligned(a.labels, 16) && dl_aligned(a.dense, 16);
}

static int dl_maps(int kind, const void* truth_maps, const void* pred_maps, int maps_kind, float alpha, DlArgs& a) {
    if (kind != PTB_DLOSS_BOUNDARY && kind != PTB_DLOSS_HAUSDORFF) return PTB_EINVAL;
    if (!truth_maps || (kind == PTB_DLOSS_HAUSDORFF) != (pred_maps != nullptr)) return PTB_EINVAL;
    if (maps_kind != PTB_DLOSS_MAPS_I32_SQUARED && maps_kind != PTB_DLOSS_MAPS_F32) return PTB_EINVAL;
    if (kind == PTB_DLOSS_HAUSDORFF && !(alpha > 0.0f && std::isfinite(alpha))) return PTB_EINVAL;
    a.phi_t = truth_maps; a.phi_p = pred_maps; a.maps_f32 = maps_kind == PTB_DLOSS_MAPS_F32; a.alpha = alpha; a.amode = alpha == 2.0f ? 2 : alpha == 1.0f ? 1 : 0;
    return PTB_OK;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_dloss_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int K, int planes, int64_t max_workspace_bytes,
                              int64_t* entries_per_chunk, int64_t* workspace_bytes, int64_t* min_workspace_bytes, int64_t* partial_slots) {
    if (int rc = edt_check_shape(dims, 1, D, H, W)) return rc;
    if (B < 1 || K < 1 || (planes != 1 && planes != 2) || max_workspace_bytes < 0) return PTB_EINVAL;
    const long long S = D * H * W;
    if (B > 0x7fffffffLL || B * dl_blocks_per_sample(S) > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    if (partial_slots) *partial_slots = B * dl_blocks_per_sample(S);
    const long long E = (long long)planes * B * K;                             // (< 2^63: each factor is below 2^31, planes <= 2)
    // a chunk starts where its int32 / float32 output is 16-byte aligned: every `step` entries
    const long long step = S % 4 == 0 ? 1 : S % 2 == 0 ? 2 : 4;
    const long long least = std::min(E, step);
    if (least > MAX_POS / S) return PTB_EUNSUPPORTED;
    auto bytes_of = [&](long long entries) {
        int64_t n = 0;
        ptb_edt_plan(dims, entries, D, H, W, 1, &n);
        return (long long)n;
    };
    if (min_workspace_bytes) *min_workspace_bytes = bytes_of(least);
    if (bytes_of(least) > max_workspace_bytes) return PTB_EINVAL;
    // the workspace grows with the entries: the largest count within the cap and ptb_edt's 2^31 - 2 positions, by bisection
    long long lo = least, hi = std::min(E, (long long)(MAX_POS / S));
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (bytes_of(mid) <= max_workspace_bytes) lo = mid;
        else hi = mid - 1;
    }
    if (lo < E) lo -= lo % step;
    if (entries_per_chunk) *entries_per_chunk = lo;
    if (workspace_bytes) *workspace_bytes = bytes_of(lo);
    return PTB_OK;
}

extern "C" int ptb_dloss_masks(const float* logits, const int64_t* labels, const float* dense, const int* classes, const int* class_table, int planes,
                               int B, int C, int K, int64_t S, int prob, int has_ignore, int64_t ignore_label, float ignore_value, uint8_t* masks,
                               ptb_stream_t stream) {
    DlArgs a{};
    if (!masks || planes < 1 || planes > (PTB_DLOSS_PLANE_TRUTH | PTB_DLOSS_PLANE_PRED)) return PTB_EINVAL;
    const bool truth = planes & PTB_DLOSS_PLANE_TRUTH, pred = planes & PTB_DLOSS_PLANE_PRED;
    if (int rc = dl_common(logits, pred, labels, dense, classes, class_table, B, C, K, S, prob, a)) return rc;      // (the truth plane alone reads no logits)
    a.has_ignore = has_ignore != 0; a.ignore_label = ignore_label; a.ignore_value = ignore_value;
    const size_t plane = (size_t)B * K * S;
    a.mask_t = truth ? masks : nullptr;
    a.mask_p = pred ? masks + (truth ? plane : 0) : nullptr;
    const bool wide = dl_wide_inputs(a) && dl_aligned(masks, 4);
    auto launch = [&](auto cr) {
        with_bool(wide, [&](auto w) {
            hipLaunchKernelGGL((dl_mask_kernel<cr(), w()>), dim3((unsigned)B * a.bps), dim3(DL_THREADS), 0, (hipStream_t)stream, a);
        });
    };
    if (pred) dl_with_channels(prob, C, launch);
    else launch(int_c<-1>{});
    return check_launch();
}

extern "C" int ptb_dloss_fwd(int kind, const float* logits, const int64_t* labels, const float* dense, const int* classes, const int* class_table,
                             const void* truth_maps, const void* pred_maps, int maps_kind, int B, int C, int K, int64_t S, int prob, int has_ignore,
                             int64_t ignore_label, float ignore_value, float alpha, int per_sample, void* workspace, int64_t workspace_bytes,
                             float* loss, float* inv_count, int* error_flag, ptb_stream_t stream) {
    DlArgs a{};
    if (!workspace || !loss || !inv_count || !error_flag) return PTB_EINVAL;
    if (int rc = dl_common(logits, true, labels, dense, classes, class_table, B, C, K, S, prob, a)) return rc;
    if (int rc = dl_maps(kind, truth_maps, pred_maps, maps_kind, alpha, a)) return rc;
    const long long slots = (long long)B * a.bps;
    if (!aligned16(workspace) || workspace_bytes < 16 * slots) return PTB_EINVAL;
    a.has_ignore = has_ignore != 0; a.ignore_label = ignore_label; a.ignore_value = ignore_value;
    a.psum = reinterpret_cast<double*>(workspace);
    a.pcnt = reinterpret_cast<long long*>(workspace) + slots;
    a.flag = error_flag;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(error_flag, 0, sizeof(int), st); e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    const bool wide = dl_wide_inputs(a) && dl_aligned(truth_maps, 16) && dl_aligned(pred_maps, 16);
    with_value<PTB_DLOSS_BOUNDARY, PTB_DLOSS_HAUSDORFF>(kind, [&](auto kd) {
        dl_with_channels(prob, C, [&](auto cr) {
            with_bool(wide, [&](auto w) {
                hipLaunchKernelGGL((dl_fwd_kernel<kd(), cr(), w()>), dim3((unsigned)slots), dim3(DL_THREADS), 0, st, a);
            });
        });
    });
    DlFinishArgs f{};
    f.psum = a.psum; f.pcnt = a.pcnt; f.loss = loss; f.inv_count = inv_count; f.flag = labels ? error_flag : nullptr;
    f.per_result = per_sample ? a.bps : (unsigned)slots;
    hipLaunchKernelGGL(dl_finish_kernel, dim3(per_sample ? (unsigned)B : 1u), dim3(DL_THREADS), 0, st, f);
    return check_launch();
}

extern "C" int ptb_dloss_bwd(int kind, const float* logits, const int64_t* labels, const float* dense, const int* classes, const int* class_table,
                             const void* truth_maps, const void* pred_maps, int maps_kind, int B, int C, int K, int64_t S, int prob, int has_ignore,
                             int64_t ignore_label, float ignore_value, float alpha, int per_sample, const float* coef, float* grad,
                             ptb_stream_t stream) {
    DlArgs a{};
    if (!coef || !grad) return PTB_EINVAL;
    if (int rc = dl_common(logits, true, labels, dense, classes, class_table, B, C, K, S, prob, a)) return rc;
    if (int rc = dl_maps(kind, truth_maps, pred_maps, maps_kind, alpha, a)) return rc;
    a.has_ignore = has_ignore != 0; a.ignore_label = ignore_label; a.ignore_value = ignore_value;
    a.coef = coef; a.grad = grad; a.per_sample = per_sample != 0;
    const bool wide = dl_wide_inputs(a) && dl_aligned(truth_maps, 16) && dl_aligned(pred_maps, 16) && dl_aligned(grad, 16);
    with_value<PTB_DLOSS_BOUNDARY, PTB_DLOSS_HAUSDORFF>(kind, [&](auto kd) {
        dl_with_channels(prob, C, [&](auto cr) {
            with_bool(wide, [&](auto w) {
                hipLaunchKernelGGL((dl_bwd_kernel<kd(), cr(), w()>), dim3((unsigned)B * a.bps), dim3(DL_THREADS), 0, (hipStream_t)stream, a);
            });
        });
    });
    return check_launch();
}
