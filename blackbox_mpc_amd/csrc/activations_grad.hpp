// Derivatives of the Dense-layer activations of activations.hpp, one definition for every kernel that differentiates a
// network (plan gradients, kernels_plan_grad.hpp).
//
// act_grad(x, y, act) is d act(x) / dx, written in the forward's own quantities: the pre-activation x and the value
// y = act(x) the forward has just computed, so tanh, sigmoid, elu, selu, softsign, exponential and swish cost a few
// multiply-adds on top of the forward and no second transcendental (swish and softplus take one v_exp_f32 / v_rcp_f32 pair
// for sigma(x)).  The absolute error is that of y, ~1e-7 .. 2.5e-7 of an O(1) value (activations.hpp).
//
// Kinks.  relu, relu6, leaky_relu and hard_sigmoid are piecewise linear; at a kink the derivative is the slope of the
// branch the forward's comparison takes there:
//   relu          x <= 0 ? 0 : x                   x > 0 ? 1 : 0          (at 0 the forward returns the constant 0)
//   relu6         x < 0 ? 0 : (x > 6 ? 6 : x)      0 at x < 0 and x > 6, else 1   (at 0 and at 6 the forward returns x)
//   leaky_relu    fmaxf(x, 0.2 x)                  x > 0 ? 1 : 0.2
//   hard_sigmoid  t = 0.2 x + 0.5 clipped          0 at t < 0 and t > 1, else 0.2  (at t = 0 and t = 1 the forward returns t)
// elu and selu are differentiable at 0 in value only for elu (selu's slopes differ: lambda against lambda alpha); both
// follow the forward's `x > 0`.  tests/plan_gradient_util.py states the same table in float64.
#pragma once
#include "activations.hpp"

namespace bbmpc {

__device__ __forceinline__ float act_grad(float x, float y, int act) {
    switch (act) {
    case ACT_TANH: return 1.0f - y * y;
    case ACT_RELU: return x > 0.0f ? 1.0f : 0.0f;
    case ACT_SIGMOID: return y * (1.0f - y);
    case ACT_ELU: return x > 0.0f ? 1.0f : y + 1.0f;                                  // e^x = y + 1
    case ACT_SELU: return x > 0.0f ? 1.0507009873554805f : y + 1.7580993408473766f;   // lambda alpha e^x = y + lambda alpha
    case ACT_SOFTPLUS: return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-BB_LOG2E * x));      // sigma(x)
    case ACT_SOFTSIGN: {
        const float r = 1.0f - __builtin_fabsf(y);                                    // 1 / (1 + |x|)
        return r * r;
    }
    case ACT_EXPONENTIAL: return y;
    case ACT_HARD_SIGMOID: {
        const float t = 0.2f * x + 0.5f;
        return t < 0.0f ? 0.0f : (t > 1.0f ? 0.0f : 0.2f);
    }
    case ACT_SWISH: {
        const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-BB_LOG2E * x));
        return s + y * (1.0f - s);                                                    // sigma + x sigma (1 - sigma)
    }
    case ACT_LEAKY_RELU: return x > 0.0f ? 1.0f : 0.2f;
    case ACT_RELU6: return x < 0.0f ? 0.0f : (x > 6.0f ? 0.0f : 1.0f);
    default: return 1.0f;
    }
}

}  // namespace bbmpc
