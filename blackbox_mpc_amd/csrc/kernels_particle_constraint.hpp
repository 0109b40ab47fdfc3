// Chance constraint of the particle evaluator (bbmpc_set_chance_constraint): a state box that does
// not end a rollout -- the share of a candidate's particles that ever leave it becomes a penalty on the candidate's score.
//
// The TRAJ form of the learned model's particle rollout (kernels_mlp_particles.hpp) has left the NOISY next state of every
// (candidate, particle) row and step in traj [H][A][S][RS], feature-major, the row's slot its returns index r = n * P + p.
// Per agent a and row r, with s_t = plane t - 1 of the row (s_0, the agent's state, is not tested):
//     out(s)      = any i: s[i] < lo[i] or s[i] > hi[i]        (both comparisons false on NaN: a NaN state violates nothing)
//     first[a][r] = the smallest t in 1 .. H with out(s_t), else 0                                    k_particle_box_scan
// and per candidate n, behind the unchanged aggregate (kernels_particles.hpp), which has left score in rewards[a][n]:
//     v           = (float)#{p : first[a][n * P + p] != 0} / (float)P
//     rewards     = score - lambda * max(0, v - delta)         (fp32, one rounding per operation)      k_particle_constraint_apply
//
// k_particle_box_scan: one lane per row, one wave per workgroup (grid = ceil(n_pop * P / 64) x A), so what is uniform in a
// wave is uniform in the workgroup and no barrier is needed anywhere.  Per step and feature the wave reads 64 consecutive
// floats of one feature row (256 bytes).  The walk over (t, feature) is cut into chunks of PCS_CHUNK features that never
// cross a plane; the loads of chunk k + 1 -- the first chunk of plane t + 1 behind the last of plane t -- are issued before
// chunk k is compared, so no step waits for a plane it has only just asked for.  Two forms:
//   REWARD = false (a HIP-source reward: rtc.hpp's bbmpc_user_reward_particles has written the returns): the box alone, no
//       LDS; the wave stops reading planes once every live lane has violated.
//   REWARD = true (a built-in reward: the TRAJ rollout computes none): every lane also keeps s_t and s_{t+1} in LDS rows of
//       its own, S | 1 floats apart (an odd stride: 64 lanes on 64 different banks), the row pointers reward_generic asks
//       for, and sums r = reward_generic(s_t, a_t, s_{t+1}) in ascending t, a_t from particle_action (which clips when `pen`
//       is set).  NaN -> -1e6 per particle, returns [A][RS].  A lane reads only the rows it wrote itself.  The actions of
//       step t are asked for when plane t's first chunk is, PCS_ACT of them in registers (the rest at the use).
// Rows r >= n_pop * P and the padding up to RS are neither read nor written.  Offsets into traj are 32 bit
// (Engine::require_particle_traj_fits).  No atomics: equal inputs give equal bits.
#pragma once
#include "kernels_particles.hpp"

namespace bbmpc {

constexpr int PCS_LANES = 64;
constexpr int PCS_CHUNK = 8;      // features per chunk of the walk
constexpr int PCS_ACT = 8;        // action elements of a step held in registers across its plane

struct ParticleConstraintArgs {
    ParticleArgs p;               // the rollout's arguments: traj, returns, rewards, the action source
    const float* box;             // [2][S]: lo | hi, -inf / +inf = unbounded
    int* first;                   // [A][RS]
    float* viol;                  // [A][Nst]
    float delta, lambda;
};

// floats of dynamic LDS of the REWARD form: two state rows and one action row per lane
__host__ __device__ inline int particle_box_scan_lds_floats(int S, int U) { return PCS_LANES * (2 * (S | 1) + (U | 1)); }

template <bool REWARD>
__global__ __launch_bounds__(PCS_LANES) void k_particle_box_scan(ParticleConstraintArgs c) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ParticleArgs& q = c.p;
    const int lane = threadIdx.x, a = blockIdx.y, r = blockIdx.x * PCS_LANES + lane;
    const int S = q.S, U = q.U, H = q.H, RS = q.RS;
    const bool live = r < q.n_pop * q.P;
    const int n = live ? r / q.P : 0;
    const float* __restrict__ lo = c.box;
    const float* __restrict__ hi = c.box + S;
    const int ld = S | 1, lu = U | 1;
    [[maybe_unused]] float* cur = smem + lane * ld;
    [[maybe_unused]] float* nxt = smem + (PCS_LANES + lane) * ld;
    [[maybe_unused]] float* act = smem + 2 * PCS_LANES * ld + lane * lu;
    if constexpr (REWARD) {
        if (live)
            for (int i = 0; i < S; ++i) cur[i] = q.state[(size_t)a * S + i];
    }
    // feature i of plane t of this row: base[t * plane_stride + i * RS]
    const float* __restrict__ base = q.traj + (size_t)a * S * RS + r;
    const int plane_stride = q.A * S * RS;
    auto load_chunk = [&](int t, int i0, float (&x)[PCS_CHUNK]) {
        const float* src = base + t * plane_stride + i0 * RS;
#pragma unroll
        for (int k = 0; k < PCS_CHUNK; ++k) x[k] = (live && i0 + k < S) ? src[k * RS] : 0.0f;
    };
    auto load_actions = [&](int t, float (&x)[PCS_ACT]) {
#pragma unroll
        for (int k = 0; k < PCS_ACT; ++k) x[k] = (live && k < U) ? particle_action(q, a, n, t, k) : 0.0f;
    };
    float v[PCS_CHUNK], w[PCS_CHUNK];
    [[maybe_unused]] float an[PCS_ACT];
    int first = 0;
    float total = 0.0f;
    load_chunk(0, 0, v);
    if constexpr (REWARD) load_actions(0, an);
    int t = 0, i0 = 0;
    for (;;) {
        int tn = t, in = i0 + PCS_CHUNK;                       // the chunk behind this one
        if (in >= S) {
            in = 0;
            tn = t + 1;
        }
        const bool more = tn < H;
        if (more) load_chunk(tn, in, w);
        bool out = false;
#pragma unroll
        for (int k = 0; k < PCS_CHUNK; ++k) {
            const int i = i0 + k;
            if (i < S) {
                const float x = v[k];
                out = out || x < lo[i] || x > hi[i];
                if constexpr (REWARD) {
                    if (live) nxt[i] = x;
                }
            }
        }
        if (out && first == 0) first = t + 1;
        if (in == 0) {                                         // plane t is complete
            if constexpr (REWARD) {
                if (live) {
#pragma unroll
                    for (int k = 0; k < PCS_ACT; ++k)
                        if (k < U) act[k] = an[k];
                    for (int u = PCS_ACT; u < U; ++u) act[u] = particle_action(q, a, n, t, u);
                    total = total + reward_generic(q.reward_kind, q.fix_q1 != 0, cur, act, nxt, S, U);
                }
                float* sw = cur; cur = nxt; nxt = sw;
                if (more) load_actions(tn, an);
            } else if (__ballot(live && first == 0) == 0) {
                break;                                         // (one wave: uniform)
            }
        }
        if (!more) break;
#pragma unroll
        for (int k = 0; k < PCS_CHUNK; ++k) v[k] = w[k];
        t = tn;
        i0 = in;
    }
    if (!live) return;
    c.first[(size_t)a * RS + r] = first;
    if constexpr (REWARD) {
        if (total != total) total = -1.0e6f;                    // deterministic.py:75-77, per particle
        q.returns[(size_t)a * RS + r] = total;
    }
}

// One lane per (candidate, agent), behind the aggregate: the candidate's P slots of `first` in index order, no atomics.
// grid (ceil(n_pop / 256), A)
static __global__ void k_particle_constraint_apply(ParticleConstraintArgs c) {
    const ParticleArgs& q = c.p;
    const int a = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= q.n_pop) return;
    const int* f = c.first + (size_t)a * q.RS + (size_t)n * q.P;
    int count = 0;
    for (int p = 0; p < q.P; ++p) count += f[p] != 0 ? 1 : 0;
    const float v = (float)count / (float)q.P;
    const size_t o = (size_t)a * q.Nst + n;
    c.viol[o] = v;
    const float excess = fmaxf(0.0f, v - c.delta);
    q.rewards[o] = q.rewards[o] - c.lambda * excess;
}

}  // namespace bbmpc
