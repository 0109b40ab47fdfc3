// Trajectory distributions (bbmpc_predict_trajectory_particles): the particle recurrence of
// kernels_particles.hpp from every row's OWN start state, every state and reward kept,
//     s_0 = states[b];  nxt = predict_next_state(s_t, seq[b, t]) + sigma (.) eps[b, p, t, :]
//     particle_states[b, p, t] = nxt;  particle_rewards[b, p, t] = reward(s_t, seq[b, t], nxt);  s_{t+1} = nxt
// and the per-step moments over the particles,
//     mean[b, t, f] = (sum_p x) / P        std[b, t, f] = sqrt(sum_p (x - mean)^2 / P)        (fp32, p in index order)
// as k_particle_aggregate forms them of the returns.  Actions are used as given, per-step values are stored as computed
// (no clip, no penalty, no NaN rule), as bbmpc_predict_trajectories does.  The analytic pendulum rolls one (b, p) row per
// lane (below); the learned model's rows go through the matrix cores (kernels_mlp_traj_particles.hpp, compiled in the
// bbmpc_mlp unit).  Nearest-rank quantiles over the particles (bbmpc_predict_trajectory_quantiles) are at the end.  Offsets into the noise and the particle tensors are 32 bit: the host refuses B * P * Hq * S >= 2^31.
#pragma once
#include "kernels_particles.hpp"
#include "traj_particle_args.hpp"

namespace bbmpc {

// One lane per (b, p) row, state in registers, the op-for-op step whatever BBMPC_STRICT_MATH says (the carried-angle form
// has no state to add the noise to); the action and the three noise elements of step t + 1 are fetched while step t
// computes.  grid (ceil(B * P / blockDim.x))
static __global__ void k_traj_pendulum_particles(TrajParticleArgs q) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= q.B * q.P) return;
    const int b = r / q.P;
    const int Hq = q.Hq;
    float s[3] = {q.states[(size_t)b * 3 + 0], q.states[(size_t)b * 3 + 1], q.states[(size_t)b * 3 + 2]};
    const float sg0 = q.sigma[0], sg1 = q.sigma[1], sg2 = q.sigma[2];
    const float* act = q.seq + (size_t)b * Hq;
    const float* eps = q.eps + (size_t)r * Hq * 3;            // row r = b * P + p
    float* so = q.pstates + (size_t)r * Hq * 3;
    float* ro = q.prewards + (size_t)r * Hq;
    const bool fq1 = q.fix_q1 != 0;
    float u = act[0], e0 = eps[0], e1 = eps[1], e2 = eps[2];
    for (int t = 0; t < Hq; ++t) {
        float un = 0.0f, f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
        if (t + 1 < Hq) {
            un = act[t + 1];
            f0 = eps[(t + 1) * 3 + 0]; f1 = eps[(t + 1) * 3 + 1]; f2 = eps[(t + 1) * 3 + 2];
        }
        const float rew = pendulum_step_noisy(fq1, s, u, sg0 * e0, sg1 * e1, sg2 * e2);
        so[t * 3 + 0] = s[0]; so[t * 3 + 1] = s[1]; so[t * 3 + 2] = s[2];
        ro[t] = rew;
        u = un; e0 = f0; e1 = f1; e2 = f2;
    }
}

// mean and std over the P values x[p * stride], p in index order
__device__ __forceinline__ void particle_moments(const float* x, int P, size_t stride, float* mean_out, float* std_out) {
    const float fp = (float)P;
    float sum = 0.0f;
    for (int p = 0; p < P; ++p) sum = sum + x[(size_t)p * stride];
    const float mean = sum / fp;
    if (mean_out) *mean_out = mean;
    if (std_out) {
        float sq = 0.0f;
        for (int p = 0; p < P; ++p) {
            const float d = x[(size_t)p * stride] - mean;
            sq = sq + d * d;
        }
        *std_out = sqrtf(sq / fp);
    }
}

// One thread per output element: (b, t, f) of the state moments [B, Hq, S], behind them (b, t) of the reward moments
// [B, Hq].  No atomics: equal inputs give equal bits.  Only the outputs that are not null are written.
static __global__ void k_traj_particle_moments(const float* __restrict__ pstates, const float* __restrict__ prewards, int B, int P, int Hq,
                                               int S, float* __restrict__ smean, float* __restrict__ sstd, float* __restrict__ rmean,
                                               float* __restrict__ rstd) {
    const long ns = (smean || sstd) ? (long)B * Hq * S : 0;
    const long nr = (rmean || rstd) ? (long)B * Hq : 0;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < ns) {
        const int b = (int)(idx / (Hq * S)), j = (int)(idx - (long)b * (Hq * S));             // j = t * S + f
        particle_moments(pstates + (size_t)b * P * Hq * S + j, P, (size_t)Hq * S, smean ? smean + idx : nullptr, sstd ? sstd + idx : nullptr);
    } else if (idx - ns < nr) {
        const long i = idx - ns;
        const int b = (int)(i / Hq), t = (int)(i - (long)b * Hq);
        particle_moments(prewards + (size_t)b * P * Hq + t, P, (size_t)Hq, rmean ? rmean + i : nullptr, rstd ? rstd + i : nullptr);
    }
}

// Nearest-rank quantiles over the particles (bbmpc_predict_trajectory_quantiles): for level l the
// particle value whose stable rank (particle_rank.hpp) among the P values of (b, t, f) is r[l] -- an element of the particle
// tensor, bit for bit.  A NaN among the P values makes their ranks meaningless (particle_rank.hpp): nothing special is
// propagated, and an output whose rank no lane holds is not written.
constexpr int QUANTILE_LEVELS_MAX = 8;
struct QuantileRanks {
    int n;                            // levels, 1 .. 8
    int r[QUANTILE_LEVELS_MAX];       // each in [0, P)
};

// lane p of the wave holds x[p * stride]; for each level the lane whose rank matches stores to out[l * level_stride]
__device__ __forceinline__ void particle_quantiles(const float* x, int lane, int P, size_t stride, const QuantileRanks& lv, float* out,
                                                   size_t level_stride) {
    const float v = lane < P ? x[(size_t)lane * stride] : 0.0f;
    const int rank = particle_stable_rank(v, lane, P);
#pragma unroll
    for (int l = 0; l < QUANTILE_LEVELS_MAX; ++l)
        if (l < lv.n && lane < P && rank == lv.r[l]) out[(size_t)l * level_stride] = v;
}

// One wave per output element: (b, t, f) of the state quantiles [B, L, Hq, S], behind them (b, t) of the reward quantiles
// [B, L, Hq]; the particle stride of a lane's load is Hq * S (Hq).  No atomics.  Only the outputs that are not null are
// written.  grid (ceil(elements / QUANTILE_WAVES)), QUANTILE_WAVES * 64 threads
constexpr int QUANTILE_WAVES = 4;
static __global__ __launch_bounds__(QUANTILE_WAVES * 64) void k_traj_particle_quantiles(const float* __restrict__ pstates,
                                                                                        const float* __restrict__ prewards, int B, int P, int Hq,
                                                                                        int S, QuantileRanks lv, float* __restrict__ squant,
                                                                                        float* __restrict__ rquant) {
    const long ns = squant ? (long)B * Hq * S : 0;
    const long nr = rquant ? (long)B * Hq : 0;
    const int lane = threadIdx.x & 63;
    const long idx = (long)blockIdx.x * QUANTILE_WAVES + (threadIdx.x >> 6);
    if (idx < ns) {
        const int b = (int)(idx / (Hq * S)), j = (int)(idx - (long)b * (Hq * S));             // j = t * S + f
        particle_quantiles(pstates + (size_t)b * P * Hq * S + j, lane, P, (size_t)Hq * S, lv, squant + (size_t)b * lv.n * Hq * S + j,
                           (size_t)Hq * S);
    } else if (idx - ns < nr) {
        const long i = idx - ns;
        const int b = (int)(i / Hq), t = (int)(i - (long)b * Hq);
        particle_quantiles(prewards + (size_t)b * P * Hq + t, lane, P, (size_t)Hq, lv, rquant + (size_t)b * lv.n * Hq + t, (size_t)Hq);
    }
}

}  // namespace bbmpc
