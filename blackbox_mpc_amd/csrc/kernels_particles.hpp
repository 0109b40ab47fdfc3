// Particle trajectory evaluator (bbmpc_set_particles): every candidate is rolled out P times with
// additive Gaussian process noise on the predicted next state and the P returns are reduced to one score,
//     nxt = predict_next_state(s_t, a_t) + sigma (.) eps[a, p, t, :]      r[n, p, a] = sum_t reward(s_t, a_t, nxt)
//     score[n, a] = mean_p r - kappa * sqrt(var_p r)                     (population variance, sums in index order)
// The noise does not depend on the candidate (common random numbers): [A][P][H][S] standard normals per optimizer
// iteration, generated once by k_gen_process_noise (stream BBMPC_NOISE_PROCESS) or injected; the rollout kernels only
// read it.  Rows of one agent are (candidate, particle) pairs, row = n * P + p:
//     returns [A][Nst * P]     scores -> the optimizer's rewards [A][Nst]
// The analytic pendulum rolls one row per lane (below); the learned model's rows go through the matrix cores
// (kernels_mlp_particles.hpp, compiled in the bbmpc_mlp unit).  The rollout kernels clip where the deterministic ones do
// but store nothing except the returns: k_particle_aggregate, one thread per candidate, writes the feasible samples back
// and forms the bound penalty of PI2 / PSO / SPSA / CMA-ES, which is subtracted from the score.
#pragma once
#include "models.hpp"
#include "particle_rank.hpp"
#include "rng.hpp"

namespace bbmpc {

constexpr uint32_t NOISE_PROCESS = 11u;      // BBMPC_NOISE_PROCESS
constexpr int PARTICLES_MAX = 64;

struct ParticleArgs {
    int n_pop, P;             // candidates per agent in this launch, particles per candidate
    int A, H, U, S, HU;
    int Nst;                  // candidate stride of cand / samples / rewards / penalty_out
    int RS;                   // row stride of returns per agent (>= n_pop * P)
    int from_ref;             // 1: seq is the caller's [n_pop, A, H, U]; 0: cand is the internal layout [A][HU][Nst]
    int pen;                  // clip to the bounds (and, in the aggregate, form the penalty)
    int fix_q1, reward_kind;
    const float* state;       // [A,S]
    const float* seq;
    const float* cand;
    const float* lo;          // [U]
    const float* hi;          // [U]
    const float* sigma;       // [S] process noise standard deviation
    const float* pnoise;      // [A][P][H][S] standard normals
    float* returns;           // [A][RS]
    float* samples;           // aggregate: where the feasible candidates go (internal layout) or null
    float* rewards;           // aggregate: scores [A][Nst]
    float* penalty_out;       // aggregate: optional [A][Nst]
    // the learned model's TRAJ rollout only (a HIP-source reward): the noisy next state of every row
    // and step, feature-major [H][A][S][RS] with the row's slot its returns index n * P + p.  The last field: no other moves.
    float* traj;
};

// Element j = t * S + s of particle p, global agent ga: counter (p, ga * Qp + (j >> 2), control step, (11 << 16) | iter),
// Qp = ceil(H * S / 4) in key.q_per_agent; Box-Muller on the word pairs as BBMPC_NOISE_NORMAL.  One thread per Philox
// block writes its (up to) four elements.  out [A][P][HS]
static __global__ void k_gen_process_noise(RngKey key, uint32_t iter, int A, int P, int HS, int agent_offset, float* out) {
    const int Qp = (HS + 3) >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A * P * Qp) return;
    const int jq = idx % Qp, p = (idx / Qp) % P, a = idx / (Qp * P);
    const RngKey kk = rng_key_now(key);
    const U4 b = rng_block(kk, NOISE_PROCESS, iter, (uint32_t)p, (uint32_t)(agent_offset + a), (uint32_t)(jq * 4));
    float z[4];
    words_to_normal2(b.x, b.y, z[0], z[1]);
    words_to_normal2(b.z, b.w, z[2], z[3]);
    float* row = out + ((size_t)a * P + p) * HS;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (jq * 4 + u < HS) row[jq * 4 + u] = z[u];
}

// Action element (t, u) of candidate n as the rollout sees it.
__device__ __forceinline__ float particle_action(const ParticleArgs& q, int a, int n, int t, int u) {
    const int j = t * q.U + u;
    float x = q.from_ref ? q.seq[((size_t)n * q.A + a) * q.HU + j] : q.cand[((size_t)a * q.HU + j) * q.Nst + n];
    if (q.pen) x = clipf(x, q.lo[u], q.hi[u]);
    return x;
}

// PendulumModel::step (models.hpp, the op-for-op form) with the noise d = sigma * eps added to the predicted next state
// before the reward sees it (quirk Q1: the as-executed reward squares the NOISY next state).
__device__ __forceinline__ float pendulum_step_noisy(bool fix_q1, float (&s)[3], float u, float d0, float d1, float d2) {
    const float theta = bb_atan2f(s[1], s[0]);
    float acc = -15.0f * bb_sinf(theta + BBMPC_PI_F);
    acc = acc + 3.0f * u;
    float nthd = s[2] + acc * 0.05f;
    const float nth = theta + nthd * 0.05f;
    nthd = clipf(nthd, -8.0f, 8.0f);
    float sn, cs;
    bb_sincosf(nth, &sn, &cs);
    const float n0 = ((cs - s[0]) + s[0]) + d0;
    const float n1 = ((sn - s[1]) + s[1]) + d1;
    const float n2 = ((nthd - s[2]) + s[2]) + d2;
    float ss;
    if (fix_q1) ss = u * u;
    else ss = (n0 * n0 + n1 * n1) + n2 * n2;
    const float r = pendulum_reward_from_theta(theta, s[2], ss);
    s[0] = n0; s[1] = n1; s[2] = n2;
    return r;
}

// One lane per (candidate, particle) row of agent blockIdx.y, state in registers; the action and the three noise
// elements of step t + 1 are fetched while step t computes.  Workgroups are sized as k_rollout_pendulum's.
static __global__ void k_rollout_pendulum_particles(ParticleArgs q) {
    const int a = blockIdx.y;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= q.n_pop * q.P) return;
    const int n = r / q.P, p = r - n * q.P;
    float s[3] = {q.state[a * 3 + 0], q.state[a * 3 + 1], q.state[a * 3 + 2]};
    const float sg0 = q.sigma[0], sg1 = q.sigma[1], sg2 = q.sigma[2];
    const float* eps = q.pnoise + ((size_t)a * q.P + p) * q.H * 3;
    const bool fq1 = q.fix_q1 != 0;
    float total = 0.0f;
    float u = particle_action(q, a, n, 0, 0), e0 = eps[0], e1 = eps[1], e2 = eps[2];
    for (int t = 0; t < q.H; ++t) {
        float un = 0.0f, f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
        if (t + 1 < q.H) {
            un = particle_action(q, a, n, t + 1, 0);
            f0 = eps[(t + 1) * 3 + 0]; f1 = eps[(t + 1) * 3 + 1]; f2 = eps[(t + 1) * 3 + 2];
        }
        total = total + pendulum_step_noisy(fq1, s, u, sg0 * e0, sg1 * e1, sg2 * e2);
        u = un; e0 = f0; e1 = f1; e2 = f2;
    }
    if (total != total) total = -1.0e6f;                        // deterministic.py:75-77, per particle
    q.returns[(size_t)a * q.RS + r] = total;
}

// One thread per (candidate, agent): the P returns in index order, no atomics.  grid (ceil(n_pop / 256), A)
static __global__ void k_particle_aggregate(ParticleArgs q, float kappa) {
    const int a = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= q.n_pop) return;
    const float* r = q.returns + (size_t)a * q.RS + (size_t)n * q.P;
    const float fp = (float)q.P;
    float sum = 0.0f;
    for (int p = 0; p < q.P; ++p) sum = sum + r[p];
    const float mean = sum / fp;
    float score = mean;
    if (kappa != 0.0f) {
        float sq = 0.0f;
        for (int p = 0; p < q.P; ++p) {
            const float d = r[p] - mean;
            sq = sq + d * d;
        }
        score = mean - kappa * sqrtf(sq / fp);
    }
    if (q.pen) {
        float pen = 0.0f;
        for (int j = 0; j < q.HU; ++j) {
            const int u = j % q.U;
            const float x = q.from_ref ? q.seq[((size_t)n * q.A + a) * q.HU + j] : q.cand[((size_t)a * q.HU + j) * q.Nst + n];
            const float xf = clipf(x, q.lo[u], q.hi[u]);
            const float d = x - xf;
            pen = pen + d * d;
            if (q.samples) q.samples[((size_t)a * q.HU + j) * q.Nst + n] = xf;
        }
        const float nr = sqrtf(pen);                            // tf.norm(...)**2  pi2.py:72-75
        pen = nr * nr;
        score = score - pen;
        if (q.penalty_out) q.penalty_out[(size_t)a * q.Nst + n] = pen;
    }
    q.rewards[(size_t)a * q.Nst + n] = score;
}

// CVaR score (bbmpc_set_particle_risk): the mean of the k worst returns of a candidate,
//     sel[p] = rank[p] < k        score = (sum over the selected p, in index order) / (float)k
// rank the stable rank of particle_rank.hpp, so the selection is exact and k = P gives the bits of the kappa = 0 mean.
// One wave per (candidate, agent): lane p holds r[p] (one coalesced load), ranks it, the ballot of sel is walked in index
// order with every lane carrying the sum through lane broadcasts.  The penalty / write-back tail is k_particle_aggregate's:
// lane l clips and writes back elements l, l + 64, .. (independent writes; an element is read and written by one lane, so
// samples may alias cand), and the squared distances are added over j in index order, again carried by every lane.
// grid (ceil(n_pop / CVAR_WAVES), A), CVAR_WAVES * 64 threads: four waves fill the four SIMDs of a CU, and 1000 candidates
// still spread over 250 CUs
constexpr int CVAR_WAVES = 4;
static __global__ __launch_bounds__(CVAR_WAVES * 64) void k_particle_aggregate_cvar(ParticleArgs q, int k) {
    const int a = blockIdx.y, lane = threadIdx.x & 63;
    const int n = blockIdx.x * CVAR_WAVES + (threadIdx.x >> 6);
    if (n >= q.n_pop) return;                                   // (the whole wave)
    const float x = lane < q.P ? q.returns[(size_t)a * q.RS + (size_t)n * q.P + lane] : 0.0f;
    const int rank = particle_stable_rank(x, lane, q.P);
    float sum = 0.0f;
    for (unsigned long long m = __ballot(lane < q.P && rank < k); m; m &= m - 1) sum = sum + wave_bcast(x, __builtin_ctzll(m));
    float score = sum / (float)k;
    if (q.pen) {
        float pen = 0.0f;
        for (int j0 = 0; j0 < q.HU; j0 += 64) {
            const int j = j0 + lane;
            float d = 0.0f;
            if (j < q.HU) {
                const int u = j % q.U;
                const float c = q.from_ref ? q.seq[((size_t)n * q.A + a) * q.HU + j] : q.cand[((size_t)a * q.HU + j) * q.Nst + n];
                const float cf = clipf(c, q.lo[u], q.hi[u]);
                d = c - cf;
                if (q.samples) q.samples[((size_t)a * q.HU + j) * q.Nst + n] = cf;
            }
            const int cnt = min(64, q.HU - j0);
            for (int i = 0; i < cnt; ++i) {
                const float di = wave_bcast(d, i);
                pen = pen + di * di;
            }
        }
        const float nr = sqrtf(pen);                            // tf.norm(...)**2  pi2.py:72-75
        pen = nr * nr;
        score = score - pen;
        if (lane == 0 && q.penalty_out) q.penalty_out[(size_t)a * q.Nst + n] = pen;
    }
    if (lane == 0) q.rewards[(size_t)a * q.Nst + n] = score;
}

}  // namespace bbmpc
