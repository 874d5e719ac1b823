// What the plane unit (ptb_softskel.hip) and the volume unit (ptb_softskel3d.hip) share on the host: the caps, the checks of the class list and
// of the activation code, and the two rank-agnostic kernels of ptb_softskel.hip as host functions -- ss_finish_kernel takes slots and a
// per-class count, ss_act_bwd_kernel takes S positions; neither knows whether S = H W or D H W.  Each launches on `stream` and checks nothing.
#pragma once
#include "ptb_common.h"

namespace ptb {

constexpr int SS_CAP = 8;                        // ptb_softskel_cap(): the LDS plan of the 2-D backward; the volume unit holds k + 1 <= 9 deltas in registers
constexpr int SS_MAX_CLASSES = 32;

// classes: HOST int[K], distinct channels in [0, C) -> cls
inline int ss_classes(const int* classes, int C, int K, int (&cls)[SS_MAX_CLASSES]) {
    if (!classes || K < 1 || K > SS_MAX_CLASSES) return K > SS_MAX_CLASSES ? PTB_EUNSUPPORTED : PTB_EINVAL;
    for (int k = 0; k < K; ++k) {
        if (classes[k] < 0 || classes[k] >= C) return PTB_EINVAL;
        for (int i = 0; i < k; ++i)
            if (classes[i] == classes[k]) return PTB_EINVAL;
        cls[k] = classes[k];
    }
    return PTB_OK;
}

inline bool ss_bad_prob(int prob) { return prob != PTB_PROB_SOFTMAX && prob != PTB_PROB_SIGMOID && prob != PTB_PROB_IDENTITY; }

// loss [1] and coef [K][3] from slots [K][per_class][4] (ss_finish_kernel)
void ss_launch_finish(const double* slots, unsigned per_class, int K, float smooth, float* loss, float* coef, hipStream_t stream);

// grad [B, C, S] = upstream[0] * the activation's Jacobian applied to dp [B, K, S] (ss_act_bwd_kernel); cls: HOST int[K], already checked.
// PTB_EUNSUPPORTED when B * S does not fit one grid.
int ss_launch_act_bwd(const float* x, const float* dp, const float* upstream, float* grad, const int* cls, int K, int C, int prob, size_t B, size_t S,
                      hipStream_t stream);

}  // namespace ptb
