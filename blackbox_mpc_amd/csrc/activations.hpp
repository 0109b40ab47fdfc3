// The Dense-layer activations of DeterministicMLP (reference dynamics_functions/deterministic_mlp.py:19-24: any Keras
// activation / tf.nn elementwise function), one definition for every kernel that applies them.
//
// A leaf header: the engine's kernels include it through kernels_mlp.hpp, and the hiprtc program of the transform rollout
// (kernels_mlp_xform.hpp, rtc.hpp) receives the same text as a named header (_build.py EMBEDDED_HEADERS), so the two
// cannot drift apart.
//
// The forms follow TF 2.0.0 (the reference pins tensorflow==2.0.0) and run on the hardware transcendental units
// (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1 ulp each) with no IEEE division: an activation feeds a dot product, so the bound
// that matters is the absolute error of an O(1) value, ~1e-7.  `exponential` (and softplus for large x, which is x plus a
// vanishing term) are held to a relative bound instead.  Every form passes NaN through as NaN (the rollouts' NaN -> -1e6
// reward guard depends on it) and gives the float64 limit at +-inf.
//
// ACT_NONE .. ACT_SIGMOID keep the forms they have always had.  The codes are the BBMPC_ACT_* constants of bbmpc.h.
//
// Padding: sigmoid, softplus, exponential and hard_sigmoid give f(0) != 0, so a padded feature (a hidden tile's empty
// slots, q4s's state slots beyond dim_S, w4 / wave tiles) holds a finite nonzero value.  Every kernel packs zero operands
// for padded inputs of the next layer and never reads padded outputs into the state or the reward, so the value is
// multiplied by zero or dropped; q4s carries its padded state slots from step to step, where they grow by at most f(0) per
// step and stay finite.
#pragma once
#include <hip/hip_runtime.h>

namespace bbmpc {

constexpr int ACT_NONE = 0, ACT_TANH = 1, ACT_RELU = 2, ACT_SIGMOID = 3;
constexpr int ACT_ELU = 4, ACT_SELU = 5, ACT_SOFTPLUS = 6, ACT_SOFTSIGN = 7, ACT_EXPONENTIAL = 8, ACT_HARD_SIGMOID = 9,
              ACT_SWISH = 10, ACT_LEAKY_RELU = 11, ACT_RELU6 = 12;

constexpr float BB_LOG2E = 1.4426950408889634f;
constexpr float BB_LOG2E_LO = 1.925963033500011e-08f;   // log2(e) - (float)log2(e)
constexpr float BB_LN2 = 0.6931471805599453f;

// tanh on the hardware exp/rcp units: sign(x) * (1 - 2 / (2^{c|x|} + 1)), c = 2 log2(e): six instructions
// (v_mul with |x|, v_exp_f32, v_add, v_rcp_f32, v_fma, v_bfi).  Absolute error <= ~2.5e-7 over the whole range (v_exp_f32 /
// v_rcp_f32 are ~1 ulp); near zero the RELATIVE error grows (cancellation) but an activation feeds a dot product, where
// only absolute error matters -- it is the size of one fp32 rounding of an O(1) pre-activation.  fp32-input MFMA
// executes at the vector rate on the same datapath as VALU work (measured: step time = MFMA time + VALU time, not the
// max), so every VALU instruction shaved off the activations is matrix time gained: this form replaced
// exp(2|x|) -> 1 - 2r spelled as (|x|+|x|) * log2e, exp2, +1, rcp, r+r, 1-  (eight instructions).
__device__ __forceinline__ float bb_tanhf(float x) {
    // tanh x = 1 - 2 / (1 + e^(2x)) holds for either sign: +inf for large x -> 1 - 0, 0 for large -x -> 1 - 2; round 5 dropped the
    // |x| / copysign pair around it (one v_bfi per value: five instructions instead of six, same absolute error bound -- the
    // reciprocal's argument lies in [1, 2) for x < 0 and the cancellation near zero is the positive side's mirrored).
    const float e = __builtin_amdgcn_exp2f(2.8853900817779268f * x);
    // v_rcp_f32 (1 ulp).  __frcp_rn is the correctly rounded reciprocal, i.e. a full IEEE division: ten instructions
    // (v_div_scale x2, v_rcp, four fmas, v_div_fmas, v_div_fixup) per activation value, on the MFMAs' issue port.
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);   // NaN stays NaN (exp2(NaN) = NaN)
}

// e^x for x <= 0 (elu, selu, softplus): exp2(x log2 e) with the product rounded once.  The rounding of the product costs
// ~|x| * 4e-8 relative, and e^x itself is <= e^-|x|, so the absolute error stays below ~1.5e-8 beyond v_exp_f32's ulp.
__device__ __forceinline__ float bb_exp_neg(float x) { return __builtin_amdgcn_exp2f(x * BB_LOG2E); }

// e^x to a relative bound over the whole range (`exponential`): the product x log2 e is carried as ph + pl (pl exact by
// fma, plus x times log2 e's low part), 2^ph from v_exp_f32 and 2^pl = 1 + pl ln 2 (|pl| < 8e-6: the dropped square is
// ~3e-11).  Relative error ~2.5e-7, where exp2(x log2 e) alone loses ~|x| * 4e-8 (1.3e-6 at x = 30).  At x = +-inf the
// split is inf - inf; the select returns 2^ph there (+inf, 0).  Overflow gives inf * (1 + pl ln 2) = inf, NaN stays NaN.
__device__ __forceinline__ float bb_exp_rel(float x) {
    const float ph = x * BB_LOG2E;
    const float pl = __builtin_fmaf(x, BB_LOG2E_LO, __builtin_fmaf(x, BB_LOG2E, -ph));
    const float e = __builtin_amdgcn_exp2f(ph);
    const float r = e * __builtin_fmaf(pl, BB_LN2, 1.0f);
    return __builtin_isinf(x) ? e : r;
}

// elu (Keras alpha 1): x > 0 ? x : e^x - 1.  NaN takes the second branch: exp2(NaN) - 1 = NaN; -inf -> 0 - 1 = -1.
__device__ __forceinline__ float bb_eluf(float x) { return x > 0.0f ? x : bb_exp_neg(x) - 1.0f; }

// selu: lambda * (x > 0 ? x : alpha (e^x - 1)) with TF's alpha and lambda; -inf -> -lambda alpha.
__device__ __forceinline__ float bb_seluf(float x) {
    constexpr float lam = 1.0507009873554805f, lam_alpha = 1.7580993408473766f;   // lambda, lambda * 1.6732632423543772
    return x > 0.0f ? lam * x : __builtin_fmaf(lam_alpha, bb_exp_neg(x), -lam_alpha);
}

// softplus: log(1 + e^x) = max(x, 0) + log(1 + e^-|x|).  e^-|x| lies in (0, 1], so nothing overflows; for large x the result
// is x + (a term below e^-x), for very negative x it is log(1 + e^x) ~ e^x to an absolute ~1e-7.  NaN: NaN + NaN;
// +inf -> inf + log 1; -inf -> 0 + log 1 = 0.
__device__ __forceinline__ float bb_softplusf(float x) {
    const float t = bb_exp_neg(-__builtin_fabsf(x));
    return fmaxf(x, 0.0f) + BB_LN2 * __builtin_amdgcn_logf(1.0f + t);
}

// softsign: x / (1 + |x|) spelled copysign(1 - 1 / (1 + |x|), x): one v_rcp_f32, no division, and +-inf -> +-1 (where
// x * rcp(1 + |x|) would be inf * 0).  The cancellation near 0 costs absolute error only.
__device__ __forceinline__ float bb_softsignf(float x) {
    return __builtin_copysignf(1.0f - __builtin_amdgcn_rcpf(1.0f + __builtin_fabsf(x)), x);
}

// hard_sigmoid, Keras 2.0's: clip(0.2 x + 0.5, 0, 1) (not torch's x / 6 + 0.5).  Compares, not min / max, so that NaN
// stays NaN.
__device__ __forceinline__ float bb_hard_sigmoidf(float x) {
    const float y = 0.2f * x + 0.5f;
    return y < 0.0f ? 0.0f : (y > 1.0f ? 1.0f : y);
}

// swish / silu: x sigma(x) = x * rcp(1 + e^-x).  For x -> -inf, rcp(inf) = 0 and x * 0 would be NaN at x = -inf itself: the
// select returns the limit 0 whenever sigma underflowed (there |x sigma(x)| < 1e-36 anyway).  +inf -> inf * 1.
__device__ __forceinline__ float bb_swishf(float x) {
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-BB_LOG2E * x));
    return s == 0.0f ? 0.0f : x * s;
}

// leaky_relu with tf.nn.leaky_relu's default slope 0.2: max(x, 0.2 x) (TF 2.0 spells it the same way); NaN in both operands.
__device__ __forceinline__ float bb_leaky_reluf(float x) { return fmaxf(x, 0.2f * x); }

// relu as a compare, so that NaN stays NaN: fmaxf(NaN, 0) is 0 (v_max_f32 returns the operand that is a number), which let a
// NaN input leave a relu layer as an ordinary activation and its candidate keep a finite score.  Every other input gives
// fmaxf's bits (-0 -> +0 included).
__device__ __forceinline__ float bb_reluf(float x) { return x <= 0.0f ? 0.0f : x; }

// relu6: min(max(x, 0), 6) as compares, so that NaN stays NaN.
__device__ __forceinline__ float bb_relu6f(float x) { return x < 0.0f ? 0.0f : (x > 6.0f ? 6.0f : x); }

template <int ACT>
__device__ __forceinline__ float apply_act_ct(float x) {
    if constexpr (ACT == ACT_TANH) return bb_tanhf(x);
    else if constexpr (ACT == ACT_RELU) return bb_reluf(x);
    else if constexpr (ACT == ACT_SIGMOID) return 1.0f / (1.0f + expf(-x));
    else if constexpr (ACT == ACT_ELU) return bb_eluf(x);
    else if constexpr (ACT == ACT_SELU) return bb_seluf(x);
    else if constexpr (ACT == ACT_SOFTPLUS) return bb_softplusf(x);
    else if constexpr (ACT == ACT_SOFTSIGN) return bb_softsignf(x);
    else if constexpr (ACT == ACT_EXPONENTIAL) return bb_exp_rel(x);
    else if constexpr (ACT == ACT_HARD_SIGMOID) return bb_hard_sigmoidf(x);
    else if constexpr (ACT == ACT_SWISH) return bb_swishf(x);
    else if constexpr (ACT == ACT_LEAKY_RELU) return bb_leaky_reluf(x);
    else if constexpr (ACT == ACT_RELU6) return bb_relu6f(x);
    else return x;
}

// Run-time codes.  The code is wave-uniform (a kernel argument), so every test below is a scalar branch.
// apply_act_base: the four codes the port always had, the per-value tests the kernels were tuned with.  Kernels built for
// networks made of those codes use it alone (EXT = false), so their code is what it was before the set grew; networks with
// any later code run separate instantiations (EXT = true, the dispatcher in bbmpc_mlp.hip picks them) that add one switch
// over the later codes behind a guard.
__device__ __forceinline__ float apply_act_base(float x, int act) {
    if (act == ACT_TANH) return bb_tanhf(x);
    if (act == ACT_RELU) return bb_reluf(x);
    if (act == ACT_SIGMOID) return 1.0f / (1.0f + expf(-x));
    return x;
}

typedef float act_f32x4 __attribute__((ext_vector_type(4)));

template <int ACT>
__device__ __forceinline__ act_f32x4 act4_ct(act_f32x4 v) {
    v.x = apply_act_ct<ACT>(v.x); v.y = apply_act_ct<ACT>(v.y); v.z = apply_act_ct<ACT>(v.z); v.w = apply_act_ct<ACT>(v.w);
    return v;
}

// the codes after sigmoid on four values, one switch for the four
__device__ __forceinline__ act_f32x4 apply_act_ext4(act_f32x4 v, int act) {
    switch (act) {
    case ACT_ELU: return act4_ct<ACT_ELU>(v);
    case ACT_SELU: return act4_ct<ACT_SELU>(v);
    case ACT_SOFTPLUS: return act4_ct<ACT_SOFTPLUS>(v);
    case ACT_SOFTSIGN: return act4_ct<ACT_SOFTSIGN>(v);
    case ACT_EXPONENTIAL: return act4_ct<ACT_EXPONENTIAL>(v);
    case ACT_HARD_SIGMOID: return act4_ct<ACT_HARD_SIGMOID>(v);
    case ACT_SWISH: return act4_ct<ACT_SWISH>(v);
    case ACT_LEAKY_RELU: return act4_ct<ACT_LEAKY_RELU>(v);
    case ACT_RELU6: return act4_ct<ACT_RELU6>(v);
    default: return v;
    }
}

// every code, one value (the row kernels, a last layer's per-feature epilogue)
__device__ __forceinline__ float apply_act(float x, int act) {
    if (act <= ACT_SIGMOID) return apply_act_base(x, act);
    const act_f32x4 v = {x, x, x, x};
    return apply_act_ext4(v, act).x;       // (the three unused lanes are dead code)
}

template <bool EXT>
__device__ __forceinline__ float apply_act_rt(float x, int act) {
    if constexpr (EXT) return apply_act(x, act);
    else return apply_act_base(x, act);
}

// four values of one layer (an MFMA accumulator tile): one dispatch for the four
template <bool EXT>
__device__ __forceinline__ act_f32x4 apply_act4(act_f32x4 v, int act) {
    if (!EXT || act <= ACT_SIGMOID) {
        v.x = apply_act_base(v.x, act); v.y = apply_act_base(v.y, act); v.z = apply_act_base(v.z, act); v.w = apply_act_base(v.w, act);
        return v;
    }
    return apply_act_ext4(v, act);
}

}  // namespace bbmpc
