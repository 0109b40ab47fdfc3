// Open-loop trajectory prediction (bbmpc_predict_trajectories) for the analytic pendulum, and the squared-error
// reduction of predicted against observed trajectories (SystemDynamicsHandler.multistep_error).  The learned model's
// kernel is kernels_mlp_traj.hpp.
#pragma once
#include "models.hpp"

namespace bbmpc {

// One thread per row: s_0 = states[b], then Hq model steps under seq[b, t]; states_out[b, t] = s_{t+1} in the
// reference's (cos, sin, thdot) form, rewards_out[b, t] = the step's reward.  FASTM = the carried-angle form the
// evaluator's rollouts use by default (models.hpp), false = op for op as the reference (BBMPC_STRICT_MATH).
template <bool FASTM>
__global__ void k_traj_pendulum(const float* __restrict__ states, const float* __restrict__ seq, int batch, int Hq, int fix_q1,
                                float* __restrict__ states_out, float* __restrict__ rewards_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    Roller<FASTM> roll(fix_q1 != 0, states[(size_t)b * 3 + 0], states[(size_t)b * 3 + 1], states[(size_t)b * 3 + 2]);
    const float* a = seq + (size_t)b * Hq;
    for (int t = 0; t < Hq; ++t) {
        const float r = roll.step(a[t]);
        if (states_out) {
            float s0, s1, s2;
            if constexpr (FASTM) {
#if BBMPC_PENDULUM_HW_SIN
                s1 = PendulumTurnModel::sin_turns(roll.m.phi);
                s0 = __builtin_amdgcn_cosf(roll.m.phi);
#else
                bb_sincosf(roll.m.theta, &s1, &s0);
#endif
                s2 = roll.m.thd;
            } else {
                s0 = roll.s[0]; s1 = roll.s[1]; s2 = roll.s[2];
            }
            float* o = states_out + ((size_t)b * Hq + t) * 3;
            o[0] = s0; o[1] = s1; o[2] = s2;
        }
        if (rewards_out) rewards_out[(size_t)b * Hq + t] = r;
    }
}

// Sum over rows of (pred - obs)^2 per column j = t * S + s of [B, Hq * S], in two stages and in double precision: stage 1
// gives every workgroup TRAJ_ERR_ROWS consecutive rows, a thread walks them in order for its column; stage 2 adds the
// row blocks' partials in order.  No atomics: the same inputs give the same bits.
constexpr int TRAJ_ERR_ROWS = 64;
static __global__ void k_traj_sq_error_partial(const float* __restrict__ pred, const float* __restrict__ obs, int batch, int cols,
                                               double* __restrict__ part) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    const int r0 = blockIdx.y * TRAJ_ERR_ROWS, r1 = min(batch, r0 + TRAJ_ERR_ROWS);
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) {
        const double d = (double)pred[(size_t)r * cols + j] - (double)obs[(size_t)r * cols + j];
        acc = acc + d * d;
    }
    part[(size_t)blockIdx.y * cols + j] = acc;
}
static __global__ void k_traj_sq_error_final(const double* __restrict__ part, int blocks, int cols, double* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    double acc = 0.0;
    for (int g = 0; g < blocks; ++g) acc = acc + part[(size_t)g * cols + j];
    out[j] = acc;
}

}  // namespace bbmpc
