// Hard-example mining (losses/hard_mining.py; the reference has no counterpart): cross-entropy averaged over the hardest elements only,
// top-k % (nnU-Net's TopKLoss) or a loss threshold with a floor on the kept count (OHEM).  Which elements are kept is decided by ONE
// threshold, an order statistic of the element losses, and a radix select finds it without a sort:
//   1. hm_loss_kernel    one streaming pass over logits and target writes the fp32 element-loss MAP (4 bytes per element; ignored elements
//                        hold the all-ones pattern HM_IGNORED, which no loss >= +0 has) and takes, per selection set, the count of elements,
//                        the count above the OHEM threshold and the histogram of the top byte of the loss bits.
//   2. hm_pick_kernel    a workgroup per set: the first call derives `kept` and the ascending rank n - kept from the device-side counts; every
//                        call scans the 256 counts and fixes the next byte of the threshold key.
//      hm_hist_kernel    between the picks: the histogram of the next byte among the map entries that share the bytes fixed so far.
//   3. hm_sum_kernel     the fp64 sum of the losses above the threshold, their count and the count of entries equal to it, a slot per workgroup,
//      hm_finish_kernel  and one workgroup per set adds the slots in index order: loss, threshold, kept count, 1 / kept, the tie weight.
//   4. hm_bwd_kernel     recomputes the activation and reads the SAVED MAP for the decision: weight / kept * (p - target), zeros elsewhere.
// The OHEM rule needs no branch of its own: with at least min(min_kept, n) losses above t0 the kept set is those losses, which are the
// `count above t0` largest ones, so both rules are "the kept largest" with a `kept` computed on the device.
// Loss bits of values >= +0 order like unsigned integers.  Histograms and counts are integer atomics (exact); floating-point sums go to
// per-workgroup slots only, so a second run gives the same bits.  Lanes take four neighbouring positions as in ptb_distance_loss.hip
// (16-byte accesses in the WIDE instances, a peeled instance otherwise); a softmax keeps C <= 16 channels in registers (buckets 4 / 8 /
// 16; CR = 0: a running maximum over memory), sigmoid channels are independent elements (CR = -1).  Every grid is a function of the shape
// alone, every loop is bounded by C or a constant, no workgroup waits for another one and nothing is read back.
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"

namespace ptb {

constexpr int HM_THREADS = 256;
constexpr unsigned HM_SPAN = HM_THREADS * 4;        // positions of a sample per workgroup of the loss and backward kernels
constexpr unsigned HM_CHUNK = HM_THREADS * 16;      // map entries of a set per workgroup of the histogram and sum kernels
constexpr unsigned HM_IGNORED = 0xffffffffu;
constexpr int HM_STATE = 264;                       // unsigned words of a set's state: hist[256], then the words below
enum { HM_N = 256, HM_ABOVE, HM_KEPT, HM_RANK, HM_PREFIX };

struct HmArgs {
    const float* x;             // [B, C, S] logits
    const long long* labels;    // [B, S], or NULL ...
    const float* dense;         // ... and [B, C, S] targets in [0, 1]
    unsigned* map;              // [B, S] or [B, C, S] loss bits
    unsigned* state;            // [sets, HM_STATE]
    const float* coef;          // [sets] upstream gradient / kept
    const unsigned* select;     // [sets, 2] the cut key, the bits of the tie weight
    float* grad;                // [B, C, S]
    int* flag;
    long long ignore_label;
    float ignore_value, t0;
    unsigned S, bps;            // positions per sample; workgroups per sample
    int C, has_ignore, per_sample;
};

// ---------------------------------------------------------------------------------------------------------- four positions
template <bool WIDE, class T>
__device__ __forceinline__ void hm_load4(const T* q, unsigned p0, unsigned S, T (&v)[4], T fill) {
    if constexpr (WIDE) {                                                      // S % 4 == 0 and an aligned base: p0 < S means p0 + 3 < S
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(v, __builtin_assume_aligned(q, A), sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p0 + j < S ? q[j] : fill;
    }
}

template <bool WIDE, class T>
__device__ __forceinline__ void hm_store4(T* q, unsigned p0, unsigned S, const T (&v)[4]) {
    if constexpr (WIDE) {
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(__builtin_assume_aligned(q, A), v, sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < S) q[j] = v[j];
    }
}

// the key of a loss: its bits, +0 for -0; a NaN (infinite logits) keeps one positive pattern so that no key but HM_IGNORED has the top bit
__device__ __forceinline__ unsigned hm_key(float l) {
    const unsigned u = __float_as_uint(l);
    return (u & 0x80000000u) ? (l != l ? 0x7fc00000u : 0u) : u;
}

// ---------------------------------------------------------------------------------------------------------- softmax of four positions
// CR > 0: C <= CR channels held in registers; CR == 0: a running maximum and the sum with respect to it over memory.
template <int CR, bool WIDE>
struct HmSoftmax {
    float xr[CR > 0 ? CR : 1][4];
    float m[4], s[4];           // max_c x_c and sum_c exp(x_c - max) >= 1
    float xl[4];                // x_label (0 without a valid label)

    __device__ __forceinline__ void init(const HmArgs& a, const float* x0, unsigned p0, const long long (&lab)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xl[j] = 0.0f;
        if constexpr (CR > 0) {
#pragma unroll
            for (int c = 0; c < CR; ++c) {
                if (c < a.C) {
                    hm_load4<WIDE>(x0 + (size_t)c * a.S, p0, a.S, xr[c], 0.0f);
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
                for (int c = 0; c < CR; ++c) {
                    sum += expf(xr[c][j] - mx);
                    if (lab[j] == c) xl[j] = xr[c][j];
                }
                m[j] = mx;
                s[j] = sum;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[j] = -INFINITY;
                s[j] = 0.0f;
            }
#pragma unroll 1
            for (int c = 0; c < a.C; ++c) {
                float v[4];
                hm_load4<WIDE>(x0 + (size_t)c * a.S, p0, a.S, v, 0.0f);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (v[j] > m[j]) {
                        s[j] = s[j] * expf(m[j] - v[j]) + 1.0f;
                        m[j] = v[j];
                    } else {
                        s[j] += expf(v[j] - m[j]);
                    }
                    if (lab[j] == c) xl[j] = v[j];
                }
            }
        }
    }
};

// the labels of four positions; live: the position exists, its label is not ignored and lies in [0, C) (one outside raises the flag)
template <bool WIDE>
__device__ __forceinline__ void hm_labels(const HmArgs& a, unsigned b, unsigned p0, bool report, long long (&lab)[4], bool (&live)[4]) {
    hm_load4<WIDE>(a.labels + (size_t)b * a.S + p0, p0, a.S, lab, (long long)-1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        live[j] = WIDE || p0 + j < a.S;
        if (!live[j]) continue;
        if (a.has_ignore && lab[j] == a.ignore_label) {
            live[j] = false;
            lab[j] = -1;
        } else if (lab[j] < 0 || lab[j] >= a.C) {
            if (report) *a.flag = 1;                                           // (every writer stores the same value)
            live[j] = false;
            lab[j] = -1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- the loss pass
// counts one element of the workgroup's set: the top byte of its key, and whether it lies above the OHEM threshold
__device__ __forceinline__ void hm_count(unsigned key, unsigned t0_key, unsigned* hist, unsigned& n, unsigned& above) {
    if (key == HM_IGNORED) return;
    atomicAdd(&hist[key >> 24], 1u);
    ++n;
    above += key > t0_key;
}

template <int CR, bool WIDE>
__global__ __launch_bounds__(HM_THREADS) void hm_loss_kernel(const HmArgs a) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wcnt[2];
    hist[threadIdx.x] = 0;
    if (threadIdx.x < 2) wcnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned b = blockIdx.x / a.bps;
    const unsigned p0 = ((blockIdx.x - b * a.bps) * HM_THREADS + threadIdx.x) * 4u;
    const unsigned t0_key = __float_as_uint(a.t0);
    unsigned n = 0, above = 0;
    if (p0 < a.S) {
        const float* x0 = a.x + (size_t)b * a.C * a.S + p0;
        if constexpr (CR >= 0) {
            long long lab[4];
            bool live[4];
            hm_labels<WIDE>(a, b, p0, true, lab, live);
            HmSoftmax<CR, WIDE> sm;
            sm.init(a, x0, p0, lab);
            unsigned key[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                key[j] = live[j] ? hm_key((sm.m[j] - sm.xl[j]) + logf(sm.s[j])) : HM_IGNORED;       // both terms are >= 0: s >= 1
                hm_count(key[j], t0_key, hist, n, above);
            }
            hm_store4<WIDE>(a.map + (size_t)b * a.S + p0, p0, a.S, key);
        } else {
#pragma unroll 1
            for (int c = 0; c < a.C; ++c) {
                const size_t off = ((size_t)b * a.C + c) * a.S + p0;
                float v[4], g[4];
                unsigned key[4];
                hm_load4<WIDE>(x0 + (size_t)c * a.S, p0, a.S, v, 0.0f);
                hm_load4<WIDE>(a.dense + off, p0, a.S, g, 0.0f);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool live = (WIDE || p0 + j < a.S) && !(a.has_ignore && g[j] == a.ignore_value);
                    // max(x, 0) - x g is x (1 - g) or -x g: x g rounds to at most |x| for g <= 1, so neither term is negative
                    const float l = (fmaxf(v[j], 0.0f) - v[j] * g[j]) + log1pf(expf(-fabsf(v[j])));
                    key[j] = live ? hm_key(l) : HM_IGNORED;
                    hm_count(key[j], t0_key, hist, n, above);
                }
                hm_store4<WIDE>(a.map + off, p0, a.S, key);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        n += __shfl_down(n, d);
        above += __shfl_down(above, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n) atomicAdd(&wcnt[0], n);
        if (above) atomicAdd(&wcnt[1], above);
    }
    __syncthreads();
    unsigned* st = a.state + (size_t)(a.per_sample ? b : 0u) * HM_STATE;
    const unsigned h = hist[threadIdx.x];
    if (h) atomicAdd(&st[threadIdx.x], h);
    if (threadIdx.x < 2 && wcnt[threadIdx.x]) atomicAdd(&st[HM_N + threadIdx.x], wcnt[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------- the select
struct HmSelectArgs {
    const unsigned* map;        // [sets, per_set]
    unsigned* state;
    double* psum;               // [sets * cps] a slot per workgroup
    unsigned* pgt;
    unsigned* peq;
    unsigned per_set, cps;      // entries of a set; workgroups per set
    int shift;                  // of the byte this pass counts
    // the first pick
    int rule;
    double k;
    long long min_kept;
};

// the 16 entries of a lane: four runs of four neighbours, the runs HM_THREADS * 4 apart
template <bool WIDE, class F>
__device__ __forceinline__ void hm_entries(const HmSelectArgs& a, unsigned set, unsigned chunk, F&& f) {
    const unsigned* base = a.map + (size_t)set * a.per_set;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned e0 = chunk * HM_CHUNK + (i * HM_THREADS + threadIdx.x) * 4u;       // (per_set < 2^31: no wrap)
        if (e0 >= a.per_set) continue;
        unsigned key[4];
        hm_load4<WIDE>(base + e0, e0, a.per_set, key, HM_IGNORED);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (key[j] != HM_IGNORED) f(key[j]);
    }
}

template <bool WIDE>
__global__ __launch_bounds__(HM_THREADS) void hm_hist_kernel(const HmSelectArgs a) {
    __shared__ unsigned hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned set = blockIdx.x / a.cps, chunk = blockIdx.x - set * a.cps;
    unsigned* st = a.state + (size_t)set * HM_STATE;
    const unsigned prefix = st[HM_PREFIX];
    hm_entries<WIDE>(a, set, chunk, [&](unsigned key) {
        if ((key >> (a.shift + 8)) == prefix) atomicAdd(&hist[(key >> a.shift) & 255u], 1u);
    });
    __syncthreads();
    const unsigned h = hist[threadIdx.x];
    if (h) atomicAdd(&st[threadIdx.x], h);
}

// how many elements of a set of n are kept
__device__ __forceinline__ unsigned hm_kept(const HmSelectArgs& a, unsigned n, unsigned above) {
    if (n == 0) return 0;
    if (a.rule == PTB_HARDCE_TOPK) {
        const double v = floor((double)n * a.k / 100.0);
        const unsigned kept = v < 1.0 ? 1u : (unsigned)v;
        return kept < n ? kept : n;
    }
    const unsigned floor_ = a.min_kept < (long long)n ? (unsigned)a.min_kept : n;
    return above >= floor_ ? above : floor_;
}

__global__ __launch_bounds__(256) void hm_pick_kernel(const HmSelectArgs a) {
    __shared__ unsigned scan[256];
    unsigned* st = a.state + (size_t)blockIdx.x * HM_STATE;
    const unsigned tid = threadIdx.x;
    const unsigned h = st[tid];
    unsigned rank, prefix = 0, kept = 0;
    if (a.shift == 24) {
        const unsigned n = st[HM_N];
        kept = hm_kept(a, n, st[HM_ABOVE]);
        rank = n - kept;                                                       // ascending, 0-based: the smallest kept element
    } else {
        rank = st[HM_RANK];
        prefix = st[HM_PREFIX];
    }
    scan[tid] = h;
    __syncthreads();                                                           // (every lane has read the words it rewrites below)
    st[tid] = 0;                                                               // the next pass counts afresh
#pragma unroll
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned v = tid >= (unsigned)d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const unsigned incl = scan[tid], excl = incl - h;
    if (a.shift == 24 && tid == 0) st[HM_KEPT] = kept;
    if (h && excl <= rank && rank < incl) {                                    // one lane at most; none when nothing is kept (rank == n)
        st[HM_PREFIX] = (prefix << 8) | tid;
        st[HM_RANK] = rank - excl;
    }
}

template <bool WIDE>
__global__ __launch_bounds__(HM_THREADS) void hm_sum_kernel(const HmSelectArgs a) {
    __shared__ double wsum[HM_THREADS / 64];
    __shared__ unsigned wgt[HM_THREADS / 64], weq[HM_THREADS / 64];
    const unsigned set = blockIdx.x / a.cps, chunk = blockIdx.x - set * a.cps;
    const unsigned thr = a.state[(size_t)set * HM_STATE + HM_PREFIX];
    double sum = 0.0;
    unsigned gt = 0, eq = 0;
    hm_entries<WIDE>(a, set, chunk, [&](unsigned key) {
        if (key > thr) {
            sum += (double)__uint_as_float(key);
            ++gt;
        }
        eq += key == thr;
    });
    // the workgroup's sum: a fixed tree inside every wave, then the four waves in order
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_down(sum, d);
        gt += __shfl_down(gt, d);
        eq += __shfl_down(eq, d);
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = sum;
        wgt[threadIdx.x >> 6] = gt;
        weq[threadIdx.x >> 6] = eq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = wsum[0];
        unsigned g = wgt[0], e = weq[0];
#pragma unroll
        for (int w = 1; w < HM_THREADS / 64; ++w) {
            r += wsum[w];
            g += wgt[w];
            e += weq[w];
        }
        a.psum[blockIdx.x] = r;
        a.pgt[blockIdx.x] = g;
        a.peq[blockIdx.x] = e;
    }
}

struct HmFinishArgs {
    const double* psum;
    const unsigned* pgt;
    const unsigned* peq;
    const unsigned* state;
    float* loss;                // [sets]
    float* threshold;           // [sets]
    long long* kept;            // [sets]
    float* inv_kept;            // [sets]
    unsigned* select;           // [sets, 2]
    const int* flag;
    unsigned cps;
};

__global__ __launch_bounds__(HM_THREADS) void hm_finish_kernel(const HmFinishArgs a) {
    __shared__ double lsum[HM_THREADS];
    __shared__ unsigned lgt[HM_THREADS], leq[HM_THREADS];
    const size_t base = (size_t)blockIdx.x * a.cps;
    const unsigned run = (a.cps + HM_THREADS - 1) / HM_THREADS;
    const unsigned lo = min(threadIdx.x * run, a.cps), hi = min(lo + run, a.cps);
    double r = 0.0;
    unsigned g = 0, e = 0;
#pragma unroll 1
    for (unsigned i = lo; i < hi; ++i) {
        r += a.psum[base + i];
        g += a.pgt[base + i];
        e += a.peq[base + i];
    }
    lsum[threadIdx.x] = r;
    lgt[threadIdx.x] = g;
    leq[threadIdx.x] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (int i = 1; i < HM_THREADS; ++i) {
            r += lsum[i];
            g += lgt[i];
            e += leq[i];
        }
        const unsigned* st = a.state + (size_t)blockIdx.x * HM_STATE;
        const unsigned kept = st[HM_KEPT], thr = st[HM_PREFIX];
        const bool bad = a.flag && *a.flag != 0;                               // a label outside [0, C): never a finite loss
        a.kept[blockIdx.x] = kept;
        if (kept == 0) {                                                       // an empty set, or nothing above t0 and no floor
            a.loss[blockIdx.x] = bad ? NAN : 0.0f;
            a.threshold[blockIdx.x] = INFINITY;
            a.inv_kept[blockIdx.x] = 0.0f;
            a.select[blockIdx.x * 2] = HM_IGNORED;                             // no key lies above it, and the entries that equal it are ignored
            a.select[blockIdx.x * 2 + 1] = 0u;
        } else {
            // gt < kept <= gt + eq: the eq entries equal to the threshold share the kept - gt places that the larger ones leave
            const double tied = (double)(kept - g);
            a.loss[blockIdx.x] = bad ? NAN : (float)((r + tied * (double)__uint_as_float(thr)) / (double)kept);
            a.threshold[blockIdx.x] = __uint_as_float(thr);
            a.inv_kept[blockIdx.x] = (float)(1.0 / (double)kept);
            a.select[blockIdx.x * 2] = thr;
            a.select[blockIdx.x * 2 + 1] = __float_as_uint((float)(tied / (double)e));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- the gradient
template <int CR, bool WIDE>
__global__ __launch_bounds__(HM_THREADS) void hm_bwd_kernel(const HmArgs a) {
    const unsigned b = blockIdx.x / a.bps;
    const unsigned p0 = ((blockIdx.x - b * a.bps) * HM_THREADS + threadIdx.x) * 4u;
    if (p0 >= a.S) return;
    const unsigned set = a.per_sample ? b : 0u;
    const unsigned cut = a.select[set * 2];
    const float tie = __uint_as_float(a.select[set * 2 + 1]), coef = a.coef[set];
    const float* x0 = a.x + (size_t)b * a.C * a.S + p0;
    float* g0 = a.grad + (size_t)b * a.C * a.S + p0;
    // coef * weight of an entry of the saved map: 1 above the cut, the tie weight on it, 0 below it and where it is ignored
    auto weight = [&](unsigned key) { return key == HM_IGNORED ? 0.0f : key > cut ? coef : key == cut ? coef * tie : 0.0f; };
    const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (CR >= 0) {
        unsigned key[4];
        hm_load4<WIDE>(a.map + (size_t)b * a.S + p0, p0, a.S, key, HM_IGNORED);
        float w[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[j] = weight(key[j]);
            any = any || (key[j] >= cut && key[j] != HM_IGNORED);
        }
        if (!__any(any)) {                                                     // nothing kept in the whole wave (a uniform branch): the logits are not read
#pragma unroll 1
            for (int c = 0; c < a.C; ++c) hm_store4<WIDE>(g0 + (size_t)c * a.S, p0, a.S, zero);
            return;
        }
        long long lab[4];
        bool live[4];
        hm_labels<WIDE>(a, b, p0, false, lab, live);
        HmSoftmax<CR, WIDE> sm;
        sm.init(a, x0, p0, lab);
        auto channel = [&](int c, const float (&v)[4]) {
            float r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = expf(v[j] - sm.m[j]) / sm.s[j] - (lab[j] == c ? 1.0f : 0.0f);
                r[j] = w[j] != 0.0f ? w[j] * d : 0.0f;                         // (exact zeros where nothing is kept, whatever the logits hold)
            }
            hm_store4<WIDE>(g0 + (size_t)c * a.S, p0, a.S, r);
        };
        if constexpr (CR > 0) {
#pragma unroll
            for (int c = 0; c < CR; ++c)
                if (c < a.C) channel(c, sm.xr[c]);
        } else {
#pragma unroll 1
            for (int c = 0; c < a.C; ++c) {
                float v[4];
                hm_load4<WIDE>(x0 + (size_t)c * a.S, p0, a.S, v, 0.0f);
                channel(c, v);
            }
        }
    } else {
#pragma unroll 1
        for (int c = 0; c < a.C; ++c) {
            const size_t off = ((size_t)b * a.C + c) * a.S + p0;
            unsigned key[4];
            hm_load4<WIDE>(a.map + off, p0, a.S, key, HM_IGNORED);
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) any = any || (key[j] >= cut && key[j] != HM_IGNORED);
            if (!__any(any)) {
                hm_store4<WIDE>(g0 + (size_t)c * a.S, p0, a.S, zero);
                continue;
            }
            float v[4], g[4], r[4];
            hm_load4<WIDE>(x0 + (size_t)c * a.S, p0, a.S, v, 0.0f);
            hm_load4<WIDE>(a.dense + off, p0, a.S, g, 0.0f);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float w = weight(key[j]);
                r[j] = w != 0.0f ? w * (1.0f / (1.0f + expf(-v[j])) - g[j]) : 0.0f;
            }
            hm_store4<WIDE>(g0 + (size_t)c * a.S, p0, a.S, r);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// CR of a launch: the register bucket of a softmax, 0 above 16 channels, -1 for the independent channels of dense targets
template <class F>
static void hm_with_channels(bool dense, int C, F&& f) {
    if (dense) f(int_c<-1>{});
    else if (C > 16) f(int_c<0>{});
    else with_at_most<4, 8, 16>(C, f);
}

static bool hm_aligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

struct HmShape {
    long long sets, per_set, cps, bps;      // selection sets, entries of one, histogram / sum workgroups of one, loss workgroups per sample
};

// the shape part of every entry point: PTB_EINVAL for a bad one, PTB_EUNSUPPORTED for a selection set of 2^31 or more elements
static int hm_shape(bool dense, int B, int C, int64_t S, int per_sample, HmShape& h) {
    if (B < 1 || C < 1 || S < 1) return PTB_EINVAL;
    if (S > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    const long long per_sample_entries = (dense ? (long long)C : 1LL) * S;      // (< 2^62)
    h.sets = per_sample ? B : 1;
    if (per_sample_entries > 0x7fffffffLL / (per_sample ? 1 : B)) return PTB_EUNSUPPORTED;
    h.per_set = per_sample_entries * (per_sample ? 1 : B);
    h.cps = (h.per_set + HM_CHUNK - 1) / HM_CHUNK;
    h.bps = (S + HM_SPAN - 1) / HM_SPAN;
    if (h.sets * h.cps > 0x7fffffffLL || (long long)B * h.bps > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    return PTB_OK;
}

static long long hm_workspace(const HmShape& h) { return h.sets * h.cps * 16 + h.sets * HM_STATE * 4; }

}  // namespace ptb

using namespace ptb;

extern "C" int64_t ptb_hardce_workspace_bytes(int dense, int B, int C, int64_t S, int per_sample) {
    HmShape h{};
    if (int rc = hm_shape(dense != 0, B, C, S, per_sample, h)) return rc;
    return hm_workspace(h);
}

extern "C" int ptb_hardce_fwd(const float* logits, const int64_t* labels, const float* dense, int B, int C, int64_t S, int has_ignore,
                              int64_t ignore_label, float ignore_value, int per_sample, int rule, double k_percent, float t0, int64_t min_kept,
                              float* map, void* workspace, int64_t workspace_bytes, float* loss, float* threshold, int64_t* kept, float* inv_kept,
                              void* select, int* error_flag, ptb_stream_t stream) {
    if (!logits || (labels != nullptr) == (dense != nullptr)) return PTB_EINVAL;
    if (!map || !workspace || !loss || !threshold || !kept || !inv_kept || !select || !error_flag) return PTB_EINVAL;
    if (rule == PTB_HARDCE_TOPK) {
        if (!(k_percent > 0.0 && k_percent <= 100.0)) return PTB_EINVAL;
    } else if (rule == PTB_HARDCE_OHEM) {
        if (!(t0 > 0.0f && std::isfinite(t0)) || min_kept < 0) return PTB_EINVAL;
    } else {
        return PTB_EINVAL;
    }
    HmShape h{};
    if (int rc = hm_shape(dense != nullptr, B, C, S, per_sample, h)) return rc;
    if (!aligned16(workspace) || workspace_bytes < hm_workspace(h) || !hm_aligned(map, 4) || !hm_aligned(select, 4)) return PTB_EINVAL;
    const long long slots = h.sets * h.cps;
    HmSelectArgs s{};
    s.map = reinterpret_cast<const unsigned*>(map);
    s.psum = reinterpret_cast<double*>(workspace);
    s.pgt = reinterpret_cast<unsigned*>(s.psum + slots);
    s.peq = s.pgt + slots;
    s.state = s.peq + slots;
    s.per_set = (unsigned)h.per_set; s.cps = (unsigned)h.cps;
    s.rule = rule; s.k = k_percent; s.min_kept = min_kept;
    HmArgs a{};
    a.x = logits; a.labels = reinterpret_cast<const long long*>(labels); a.dense = dense;
    a.map = reinterpret_cast<unsigned*>(map); a.state = s.state; a.flag = error_flag;
    a.has_ignore = has_ignore != 0; a.ignore_label = ignore_label; a.ignore_value = ignore_value;
    a.t0 = rule == PTB_HARDCE_OHEM ? t0 : 0.0f;
    a.S = (unsigned)S; a.bps = (unsigned)h.bps; a.C = C; a.per_sample = per_sample != 0;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(error_flag, 0, sizeof(int), st); e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    if (hipError_t e = hipMemsetAsync(s.state, 0, (size_t)h.sets * HM_STATE * 4, st); e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    const bool wide = S % 4 == 0 && hm_aligned(logits, 16) && hm_aligned(labels, 16) && hm_aligned(dense, 16) && hm_aligned(map, 16);
    hm_with_channels(dense != nullptr, C, [&](auto cr) {
        with_bool(wide, [&](auto w) {
            hipLaunchKernelGGL((hm_loss_kernel<cr(), w()>), dim3((unsigned)(B * h.bps)), dim3(HM_THREADS), 0, st, a);
        });
    });
    const bool wide_map = h.per_set % 4 == 0 && hm_aligned(map, 16);
    const dim3 grid((unsigned)slots);
    for (int shift = 24; shift >= 0; shift -= 8) {
        s.shift = shift;
        if (shift != 24)
            with_bool(wide_map, [&](auto w) { hipLaunchKernelGGL((hm_hist_kernel<w()>), grid, dim3(HM_THREADS), 0, st, s); });
        hipLaunchKernelGGL(hm_pick_kernel, dim3((unsigned)h.sets), dim3(256), 0, st, s);
    }
    with_bool(wide_map, [&](auto w) { hipLaunchKernelGGL((hm_sum_kernel<w()>), grid, dim3(HM_THREADS), 0, st, s); });
    HmFinishArgs f{};
    f.psum = s.psum; f.pgt = s.pgt; f.peq = s.peq; f.state = s.state;
    f.loss = loss; f.threshold = threshold; f.kept = reinterpret_cast<long long*>(kept); f.inv_kept = inv_kept;
    f.select = reinterpret_cast<unsigned*>(select); f.flag = labels ? error_flag : nullptr; f.cps = (unsigned)h.cps;
    hipLaunchKernelGGL(hm_finish_kernel, dim3((unsigned)h.sets), dim3(HM_THREADS), 0, st, f);
    return check_launch();
}

extern "C" int ptb_hardce_bwd(const float* logits, const int64_t* labels, const float* dense, const float* map, int B, int C, int64_t S,
                              int per_sample, const float* coef, const void* select, float* grad, ptb_stream_t stream) {
    if (!logits || (labels != nullptr) == (dense != nullptr) || !map || !coef || !select || !grad) return PTB_EINVAL;
    HmShape h{};
    if (int rc = hm_shape(dense != nullptr, B, C, S, per_sample, h)) return rc;
    if (!hm_aligned(map, 4) || !hm_aligned(select, 4)) return PTB_EINVAL;
    HmArgs a{};
    a.x = logits; a.labels = reinterpret_cast<const long long*>(labels); a.dense = dense;
    a.map = const_cast<unsigned*>(reinterpret_cast<const unsigned*>(map));
    a.coef = coef; a.select = reinterpret_cast<const unsigned*>(select); a.grad = grad;
    a.S = (unsigned)S; a.bps = (unsigned)h.bps; a.C = C; a.per_sample = per_sample != 0;
    const bool wide = S % 4 == 0 && hm_aligned(logits, 16) && hm_aligned(labels, 16) && hm_aligned(dense, 16) && hm_aligned(map, 16) && hm_aligned(grad, 16);
    hm_with_channels(dense != nullptr, C, [&](auto cr) {
        with_bool(wide, [&](auto w) {
            hipLaunchKernelGGL((hm_bwd_kernel<cr(), w()>), dim3((unsigned)(B * h.bps)), dim3(HM_THREADS), 0, (hipStream_t)stream, a);
        });
    });
    return check_launch();
}
