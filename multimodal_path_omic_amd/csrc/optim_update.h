// The flat optimisers' per-element update: shared by optim.hip (mpo_optim_step_flat) and grad_guard.hip
// (mpo_optim_step_flat_guarded), so that the two apply one arithmetic.  The rules are stated in optim.hip.
#pragma once
#include "../../include/mpo_hip.h"

namespace {

struct OptCoef {
    float lr, b1, b2, eps, wd, l1, bc1, bc2_sqrt;
};

template <int ALG>
__device__ __forceinline__ void opt_update(float& p, float g, float& s1, float& s2, const OptCoef& c) {
    float gi = g;
    if (c.l1 != 0.0f) gi += c.l1 * (float)((p > 0.0f) - (p < 0.0f));
    gi = gi + c.wd * p;
    if constexpr (ALG == MPO_OPTIM_ADAM) {
        const float mi = c.b1 * s1 + (1.0f - c.b1) * gi;
        const float vi = c.b2 * s2 + (1.0f - c.b2) * gi * gi;
        s1 = mi;
        s2 = vi;
        p = p - (c.lr / c.bc1) * mi / (sqrtf(vi) / c.bc2_sqrt + c.eps);
    } else if constexpr (ALG == MPO_OPTIM_ADAMAX) {
        const float mi = s1 + (1.0f - c.b1) * (gi - s1);
        const float ui = fmaxf(c.b2 * s2, fabsf(gi) + c.eps);
        s1 = mi;
        s2 = ui;
        p = p - (c.lr / c.bc1) * (mi / ui);
    } else if constexpr (ALG == MPO_OPTIM_ADADELTA) {
        const float vi = c.b1 * s1 + (1.0f - c.b1) * gi * gi;
        const float d = sqrtf(s2 + c.eps) / sqrtf(vi + c.eps) * gi;
        s1 = vi;
        s2 = c.b1 * s2 + (1.0f - c.b1) * d * d;
        p = p - c.lr * d;
    } else {
        p = p - c.lr * gi;
    }
}

}  // namespace
