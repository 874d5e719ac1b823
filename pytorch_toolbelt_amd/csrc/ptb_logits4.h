// What the newer loss units share on the device and at their launch sites: ptb_distance_loss.hip, ptb_hard_mining.hip (the streaming units)
// and ptb_softskel.hip, ptb_softskel3d.hip (the tile units).  Header-inline only, so every unit compiles it under its own flags; the tuned
// kernels of ptb_losses.hip use other arithmetic (ptb_loss_device.h) and share nothing with this file.
// THE CONTRACT of the streaming units: logits are [B, C, S] fp32, a LANE TAKES FOUR NEIGHBOURING POSITIONS p0 .. p0 + 3 of one sample, and
// every pointer handed to load4 / store4 already points at position p0.
//   WIDE  S % 4 == 0 and every base is 16-byte aligned (4-byte for byte planes): p0 < S means p0 + 3 < S, one 16-byte access per array.
//         Otherwise the peeled instance tests every position and reads `fill` past the end.  The launch site decides with wide().
//   CR    how a softmax holds its channels: CR > 0 HELD, C <= CR channels in registers (buckets 4 / 8 / 16); CR == 0 SWEEP, a running
//         maximum over memory and a second pass wherever the channels are needed again; CR == -1 INDEPENDENT channels (sigmoid / identity),
//         no state at all.  The launch site decides with with_channels().  The register softmax itself stays a struct of each unit
//         (DlChannels, HmSoftmax): hard mining picks x_label inside the sweep, and a shared struct with a callback for that cost its
//         16-channel instances two registers and a wave of occupancy.
// The tile units take ONE position at a time: prob() and target() below, and block_sums() for their per-workgroup float64 sums.
#pragma once
#include <cmath>
#include <initializer_list>

#include "ptb_common.h"
#include "ptb_dispatch.h"

namespace ptb {

// ---------------------------------------------------------------------------------------------------------- four positions
template <bool WIDE, class T>
__device__ __forceinline__ void load4(const T* q, unsigned p0, unsigned S, T (&v)[4], T fill) {
    if constexpr (WIDE) {                                                      // S % 4 == 0 and an aligned base: p0 < S means p0 + 3 < S
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(v, __builtin_assume_aligned(q, A), sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p0 + j < S ? q[j] : fill;
    }
}

template <bool WIDE, class T>
__device__ __forceinline__ void store4(T* q, unsigned p0, unsigned S, const T (&v)[4]) {
    if constexpr (WIDE) {
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(__builtin_assume_aligned(q, A), v, sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < S) q[j] = v[j];
    }
}

// ---------------------------------------------------------------------------------------------------------- the labels of four positions
enum Label4 : int { LABEL_ABSENT, LABEL_IGNORED, LABEL_OUTSIDE, LABEL_VALID };     // past the end (peeled) | ignore_label | not in [0, C) | a class

// labels: [B, S] int64.  Loads the four labels of sample b at p0 (-1 past the end) and classifies each; one outside [0, C) raises *flag when
// `report`.  What counts as live is the caller's business.
template <bool WIDE>
__device__ __forceinline__ void labels4(const long long* labels, unsigned b, unsigned p0, unsigned S, int C, int has_ignore, long long ignore_label,
                                        bool report, int* flag, long long (&lab)[4], Label4 (&kind)[4]) {
    load4<WIDE>(labels + (size_t)b * S + p0, p0, S, lab, (long long)-1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!(WIDE || p0 + j < S)) kind[j] = LABEL_ABSENT;
        else if (has_ignore && lab[j] == ignore_label) kind[j] = LABEL_IGNORED;
        else if (lab[j] < 0 || lab[j] >= C) {
            if (report) *flag = 1;                                             // (every writer stores the same value)
            kind[j] = LABEL_OUTSIDE;
        } else kind[j] = LABEL_VALID;
    }
}

// ---------------------------------------------------------------------------------------------------------- one position
// the activation of channel ch at one position; x0: channel 0 of the sample at that position.  A softmax reads the C logits of the cell.
__device__ __forceinline__ float prob(const float* x0, int ch, int C, size_t S, int act) {
    const float v = x0[(size_t)ch * S];
    if (act == PTB_PROB_IDENTITY) return v;
    if (act == PTB_PROB_SIGMOID) return 1.0f / (1.0f + expf(-v));
    float m = x0[0];
#pragma unroll 1
    for (int c = 1; c < C; ++c) m = fmaxf(m, x0[(size_t)c * S]);
    float s = 0.0f;
#pragma unroll 1
    for (int c = 0; c < C; ++c) s += expf(x0[(size_t)c * S] - m);
    return expf(v - m) / s;
}

// the target of channel ch at position pos of sample b: labels [B, S] == ch, or dense [B, C, S] as it stands
__device__ __forceinline__ float target(const long long* labels, const float* dense, size_t b, int ch, int C, size_t S, size_t pos) {
    if (labels) return labels[b * S + pos] == (long long)ch ? 1.0f : 0.0f;
    return dense[(b * (size_t)C + (size_t)ch) * S + pos];
}

// The N float64 sums of a workgroup of 64 * WAVES lanes: a fixed tree inside every wave, then the waves in order.  Lane q < N returns sum q
// (the other lanes 0).  Every lane of the workgroup calls it; wsum is the workgroup's own LDS.
template <int N, int WAVES>
__device__ __forceinline__ double block_sums(double (&s)[N], double (&wsum)[WAVES][N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s[q] += __shfl_down(s[q], d);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < N) {
        r = wsum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) r += wsum[w][threadIdx.x];
    }
    return r;
}

// ---------------------------------------------------------------------------------------------------------- host side
// CR of a launch: -1 for independent channels, else the register bucket of a softmax, 0 above 16 channels
template <class F>
void with_channels(bool independent, int C, F&& f) {
    if (independent) f(int_c<-1>{});
    else if (C > 16) f(int_c<0>{});
    else with_at_most<4, 8, 16>(C, f);
}

inline bool aligned_to(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

// WIDE of a launch over rows of S elements: every base (NULL: an array the call does not have) is 16-byte aligned
inline bool wide(long long S, std::initializer_list<const void*> bases) {
    if (S % 4 != 0) return false;
    for (const void* p : bases)
        if (!aligned_to(p, 16)) return false;
    return true;
}

}  // namespace ptb
