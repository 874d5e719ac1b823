// The model-output activations of the 3-D merge and mirror TTA (ptb_volume_activation.hip): ApplySigmoidTo / ApplySoftmaxTo of the
// reference (inference/ensembling.py:38-42, 62-66) on the C channel values of PIX voxels of one view, held in registers.
#pragma once
#include "ptb_view_device.h"

namespace ptb {

// 1 / (1 + exp(-z)): exactly 0 / 1 once exp saturates (exp2 gives inf / 0 there, never NaN)
__device__ __forceinline__ float act_sigmoid(float z) { return fast_rcp(__fadd_rn(1.0f, fast_exp(-z))); }

// v[c][j] <- f(v[c][j]) for the channel groups (four channels each) that hold a channel below nc.  One wave-uniform branch per group,
// not per channel: per-channel guards around every phase cost more registers than the few idle channels of the last group cost time.
template <int CREG, int PIX, class F>
__device__ __forceinline__ void act_each(float (&v)[CREG][PIX], int nc, F&& f) {
#pragma unroll
    for (int g = 0; g < CREG; g += 4) {
        if (g < nc) {
#pragma unroll
            for (int c = g; c < g + 4; ++c) {
#pragma unroll
                for (int j = 0; j < PIX; ++j) v[c][j] = f(v[c][j], c, j);
            }
        }
    }
}

// v[c][j] <- A(v[c][j]) for the channels c < nc (wave-uniform) of the voxels j: z = x * t rounded; sigmoid per element; softmax over the
// nc channels of a voxel: exp(z - max) summed in channel order, each term times the reciprocal of the sum.  The channels from nc to the
// end of the last group hold finite values on entry (a repeated load) and anything on exit: softmax counts them as -inf, which changes
// neither the maximum nor, as exact zeros added last, the sum.  `act` is wave-uniform.
template <int CREG, int PIX>
__device__ __forceinline__ void activate(float (&v)[CREG][PIX], int nc, int act, float t) {
    if (act == PTB_ACT_NONE) return;
    if (act == PTB_ACT_SIGMOID) {
        act_each(v, nc, [=](float x, int, int) { return act_sigmoid(__fmul_rn(x, t)); });
        return;
    }
    float m[PIX], s[PIX];
#pragma unroll
    for (int j = 0; j < PIX; ++j) { m[j] = -INFINITY; s[j] = 0.f; }
    act_each(v, nc, [&](float x, int c, int j) {
        const float z = c < nc ? __fmul_rn(x, t) : -INFINITY;
        m[j] = fmaxf(m[j], z);
        return z;
    });
    act_each(v, nc, [&](float z, int, int j) {
        const float e = fast_exp(__fsub_rn(z, m[j]));
        s[j] = __fadd_rn(s[j], e);
        return e;
    });
#pragma unroll
    for (int j = 0; j < PIX; ++j) s[j] = fast_rcp(s[j]);
    act_each(v, nc, [&](float e, int, int j) { return __fmul_rn(e, s[j]); });
}

// v[c][j] <- red_pre(v[c][j], op) / red_post(.., op, divisor) with the wave-uniform `op` resolved once per call, not once per element
template <int CREG, int PIX>
__device__ __forceinline__ void act_red_pre(float (&v)[CREG][PIX], int nc, int op) {
    switch (op) {
        case PTB_RED_GMEAN: act_each(v, nc, [](float x, int, int) { return red_pre<1>(x, PTB_RED_GMEAN); }); break;
        case PTB_RED_HMEAN: act_each(v, nc, [](float x, int, int) { return red_pre<1>(x, PTB_RED_HMEAN); }); break;
        case PTB_RED_HARMONIC1P: act_each(v, nc, [](float x, int, int) { return red_pre<1>(x, PTB_RED_HARMONIC1P); }); break;
        case PTB_RED_LOGODD: act_each(v, nc, [](float x, int, int) { return red_pre<1>(x, PTB_RED_LOGODD); }); break;
        case PTB_RED_LOG1P: act_each(v, nc, [](float x, int, int) { return red_pre<1>(x, PTB_RED_LOG1P); }); break;
        default: break;
    }
}
template <int CREG, int PIX>
__device__ __forceinline__ void act_red_post(float (&v)[CREG][PIX], int nc, int op, float divisor) {
    switch (op) {
        case PTB_RED_GMEAN: act_each(v, nc, [=](float x, int, int) { return red_post<1>(x, PTB_RED_GMEAN, divisor); }); break;
        case PTB_RED_HMEAN: act_each(v, nc, [=](float x, int, int) { return red_post<1>(x, PTB_RED_HMEAN, divisor); }); break;
        case PTB_RED_HARMONIC1P: act_each(v, nc, [=](float x, int, int) { return red_post<1>(x, PTB_RED_HARMONIC1P, divisor); }); break;
        case PTB_RED_LOGODD: act_each(v, nc, [=](float x, int, int) { return red_post<1>(x, PTB_RED_LOGODD, divisor); }); break;
        case PTB_RED_LOG1P: act_each(v, nc, [=](float x, int, int) { return red_post<1>(x, PTB_RED_LOG1P, divisor); }); break;
        default: act_each(v, nc, [=](float x, int, int) { return red_post<0>(x, PTB_RED_SUM, divisor); }); break;
    }
}

}  // namespace ptb
