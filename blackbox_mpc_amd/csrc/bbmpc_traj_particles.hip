// Trajectory distributions (bbmpc_predict_trajectory_particles[_dev], bbmpc_predict_trajectory_quantiles[_dev];
// kernels_traj_particles.hpp, DESIGN.md sections 8e and 8f): the particle recurrence of bbmpc_set_particles from every row's
// own start state with every state and reward kept, the per-step mean / std over the particles and their nearest-rank
// quantiles.  The launch sequence  draws (unless supplied) -> noisy trajectories of every (b, p) row -> moments ->
// quantiles, and the ABI.  The learned model's trajectory kernel is launched from bbmpc_mlp.hip.
#include "abi_util.hpp"
#include "kernels_traj_particles.hpp"

namespace bbmpc {

// what the entry points refuse, before anything is allocated, copied or launched.  quantiles: the levels are checked too
// (num_levels / ranks of bbmpc_predict_trajectory_quantiles)
static void check_traj_particles(const Engine& e, int batch, int horizon, bool any_out, bool quantiles = false, int num_levels = 0,
                                 const int32_t* ranks = nullptr) {
    REQUIRE(e.particles_on(), BBMPC_E_STATE, "trajectory distribution: particles are off: call bbmpc_set_particles first");
    REQUIRE(batch >= 1, BBMPC_E_INVALID, "batch must be >= 1");
    REQUIRE(horizon >= 1 && horizon <= 4096, BBMPC_E_INVALID, "horizon must be in [1, 4096]");
    REQUIRE(any_out, BBMPC_E_INVALID, quantiles ? "all eight outputs are null" : "all six outputs are null");
    if (quantiles) {
        REQUIRE(num_levels >= 1 && num_levels <= QUANTILE_LEVELS_MAX, BBMPC_E_INVALID, "trajectory quantiles: num_levels must be in [1, 8]");
        REQUIRE(ranks != nullptr, BBMPC_E_INVALID, "null pointer argument: ranks");
        for (int l = 0; l < num_levels; ++l)
            REQUIRE(ranks[l] >= 0 && ranks[l] < e.part_P, BBMPC_E_INVALID,
                    "trajectory quantiles: rank " + std::to_string(ranks[l]) + " is outside [0, num_particles = " + std::to_string(e.part_P) + ")");
    }
    REQUIRE(!e.user_path() || e.particle_user_reward(), BBMPC_E_UNSUPPORTED, "particles with user-supplied dynamics or an inverse target transform");
    if (e.particle_user_reward()) e.require_particle_user_reward();       // a callback, or no source yet
    if (e.cfg.dynamics == BBMPC_DYN_MLP) REQUIRE(e.mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    const long qp = ((long)horizon * e.S + 3) / 4;
    REQUIRE((long)batch * e.part_P * horizon * e.S < (1L << 31) && (long)batch * horizon * e.U < (1L << 31), BBMPC_E_UNSUPPORTED,
            "trajectory distribution: more than 2^31 particle-state or action elements per call");
    REQUIRE((long)batch * qp < (1L << 32), BBMPC_E_UNSUPPORTED, "trajectory distribution: more than 2^32 noise blocks per call");
    if (quantiles)
        REQUIRE((long)batch * num_levels * horizon * e.S < (1L << 31), BBMPC_E_UNSUPPORTED,
                "trajectory quantiles: more than 2^31 quantile elements per call");
}

void Engine::roll_trajectory_particles(const float* d_states, const float* d_seq, int batch, int horizon, const float* d_eps, float*& d_pstates,
                                       float*& d_prewards) {
    const int P = part_P;
    if (particle_user_reward()) {                          // refused before anything is allocated or launched
        if (user_reward_params_dev() && rew_params.per_agent)
            REQUIRE(batch % A == 0, BBMPC_E_INVALID,
                    "per-agent runtime parameters: a call on B rows needs B to be a multiple of num_agents (B / A consecutive rows per agent)");
    }
    const size_t nps = (size_t)batch * P * horizon * S, npr = (size_t)batch * P * horizon;
    if (!d_eps) {
        // the handle's own draws: the process-noise stream with the row in the agent word, the handle's current control step,
        // iteration 0 -- at batch = A, horizon = H the tensor bbmpc_evaluate_particles rolls
        if (tjp_noise.n < nps) tjp_noise.alloc(nps);
        RngKey kk = key(step_counter);
        kk.q_per_agent = (uint32_t)((horizon * S + 3) / 4);
        kk.step_src = nullptr;
        // (k_gen_process_noise indexes its batch * P * Qp blocks in int: below 2^29 + batch * P behind check_traj_particles'
        // batch * P * horizon * S < 2^31)
        const long blocks = (long)batch * P * kk.q_per_agent;
        hipLaunchKernelGGL(k_gen_process_noise, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, stream, kk, 0u, batch, P, horizon * S,
                           cfg.agent_offset, tjp_noise.p);
        HIP_CHECK(hipGetLastError());
        d_eps = tjp_noise.p;
    }
    if (!d_pstates) {
        if (tjp_ps.n < nps) tjp_ps.alloc(nps);
        d_pstates = tjp_ps.p;
    }
    if (!d_prewards) {
        if (tjp_pr.n < npr) tjp_pr.alloc(npr);
        d_prewards = tjp_pr.p;
    }
    TrajParticleArgs q;
    memset(&q, 0, sizeof(q));
    q.B = batch; q.P = P; q.Hq = horizon; q.U = U; q.S = S;
    q.reward_kind = builtin_reward_kind();
    q.fix_q1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER) ? 1 : 0;
    q.states = d_states; q.seq = d_seq;
    q.sigma = d_psigma.p;
    q.eps = d_eps;
    q.pstates = d_pstates; q.prewards = d_prewards;
    if (cfg.dynamics == BBMPC_DYN_MLP) {
        launch_traj_mlp_particles(q);
        // a HIP-source reward: the kernel above left zeros (REW_NONE); the scorer fills prewards from
        // pstates before the moments and the quantiles read them
        if (particle_user_reward()) score_traj_particles_user(q);
    } else {
        const long rows = (long)batch * P;
        const int bs = rows <= 16384 ? 64 : 256;           // few rows: one wave per workgroup, as k_rollout_pendulum_particles
        hipLaunchKernelGGL(k_traj_pendulum_particles, dim3((unsigned)((rows + bs - 1) / bs)), dim3(bs), 0, stream, q);
        HIP_CHECK(hipGetLastError());
    }
}

// the moments that are wanted, of the particle tensors
static void launch_traj_moments(Engine& e, const float* d_pstates, const float* d_prewards, int batch, int horizon, float* d_smean, float* d_sstd,
                                float* d_rmean, float* d_rstd) {
    const int P = e.part_P, S = e.S;
    hipStream_t stream = e.stream;
    if (d_smean || d_sstd || d_rmean || d_rstd) {
        const long n = ((d_smean || d_sstd) ? (long)batch * horizon * S : 0) + ((d_rmean || d_rstd) ? (long)batch * horizon : 0);
        hipLaunchKernelGGL(k_traj_particle_moments, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const float*)d_pstates,
                           (const float*)d_prewards, batch, P, horizon, S, d_smean, d_sstd, d_rmean, d_rstd);
        HIP_CHECK(hipGetLastError());
    }
}

void Engine::predict_trajectory_particles_dev(const float* d_states, const float* d_seq, int batch, int horizon, const float* d_eps,
                                              float* d_smean, float* d_sstd, float* d_rmean, float* d_rstd, float* d_pstates, float* d_prewards) {
    check_traj_particles(*this, batch, horizon, d_smean || d_sstd || d_rmean || d_rstd || d_pstates || d_prewards);
    roll_trajectory_particles(d_states, d_seq, batch, horizon, d_eps, d_pstates, d_prewards);
    launch_traj_moments(*this, d_pstates, d_prewards, batch, horizon, d_smean, d_sstd, d_rmean, d_rstd);
}

void Engine::predict_trajectory_quantiles_dev(const float* d_states, const float* d_seq, int batch, int horizon, const float* d_eps, float* d_smean,
                                              float* d_sstd, float* d_rmean, float* d_rstd, float* d_pstates, float* d_prewards, int num_levels,
                                              const int32_t* ranks, float* d_squant, float* d_rquant) {
    check_traj_particles(*this, batch, horizon, d_smean || d_sstd || d_rmean || d_rstd || d_pstates || d_prewards || d_squant || d_rquant, true,
                         num_levels, ranks);
    roll_trajectory_particles(d_states, d_seq, batch, horizon, d_eps, d_pstates, d_prewards);
    launch_traj_moments(*this, d_pstates, d_prewards, batch, horizon, d_smean, d_sstd, d_rmean, d_rstd);
    if (d_squant || d_rquant) {
        QuantileRanks lv;
        memset(&lv, 0, sizeof(lv));
        lv.n = num_levels;
        for (int l = 0; l < num_levels; ++l) lv.r[l] = ranks[l];
        const long n = (d_squant ? (long)batch * horizon * S : 0) + (d_rquant ? (long)batch * horizon : 0);      // one wave each
        hipLaunchKernelGGL(k_traj_particle_quantiles, dim3((unsigned)((n + QUANTILE_WAVES - 1) / QUANTILE_WAVES)), dim3(QUANTILE_WAVES * 64), 0,
                           stream, (const float*)d_pstates, (const float*)d_prewards, batch, part_P, horizon, S, lv, d_squant, d_rquant);
        HIP_CHECK(hipGetLastError());
    }
}

// The host variants: stage the inputs and the outputs that are wanted in one device buffer, run the _dev form, copy back.
// quantiles false: bbmpc_predict_trajectory_particles (outs[6], outs[7] null, the levels are not read)
static void traj_particles_host(Engine& e, const float* states, const float* seq, int batch, int horizon, const float* eps, bool quantiles,
                                int num_levels, const int32_t* ranks, float* const (&outs)[8]) {
    bool any = false;
    for (int i = 0; i < 8; ++i) any = any || outs[i];
    check_traj_particles(e, batch, horizon, any, quantiles, num_levels, ranks);
    const size_t P = (size_t)e.part_P;
    const size_t ns = (size_t)batch * e.S, nq = (size_t)batch * horizon * e.U, nm = (size_t)batch * horizon * e.S, nr = (size_t)batch * horizon;
    const size_t nps = nm * P, npr = nr * P;
    // the slots are declared in the order of the arguments; an output that is not wanted gives a null slot
    const size_t nl = quantiles ? (size_t)num_levels : 0;
    const size_t sizes[8] = {nm, nm, nr, nr, nps, npr, nm * nl, nr * nl};
    HostStage st(e);
    const int s = st.in(states, ns), q = st.in(seq, nq), ep = st.in(eps, nps);
    int o[8];
    float* d[8];                                                              // the outputs' slots and device pointers
    for (int i = 0; i < 8; ++i) o[i] = st.out(outs[i], sizes[i]);
    st.upload();
    for (int i = 0; i < 8; ++i) d[i] = st[o[i]];
    if (quantiles)
        e.predict_trajectory_quantiles_dev(st[s], st[q], batch, horizon, st[ep], d[0], d[1], d[2], d[3], d[4], d[5], num_levels, ranks, d[6], d[7]);
    else
        e.predict_trajectory_particles_dev(st[s], st[q], batch, horizon, st[ep], d[0], d[1], d[2], d[3], d[4], d[5]);
    st.finish();
}

}  // namespace bbmpc

extern "C" {

int bbmpc_predict_trajectory_particles_dev(bbmpc_handle h, const float* d_states, const float* d_seq, int32_t batch, int32_t horizon,
                                           const float* d_eps, float* d_state_mean, float* d_state_std, float* d_reward_mean,
                                           float* d_reward_std, float* d_particle_states, float* d_particle_rewards) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    CHECK_PTR(d_seq);
    h->e->predict_trajectory_particles_dev(d_states, d_seq, batch, horizon, d_eps, d_state_mean, d_state_std, d_reward_mean, d_reward_std,
                                           d_particle_states, d_particle_rewards);
    API_END
}

int bbmpc_predict_trajectory_particles(bbmpc_handle h, const float* states, const float* seq, int32_t batch, int32_t horizon,
                                       const float* eps, float* state_mean, float* state_std, float* reward_mean, float* reward_std,
                                       float* particle_states, float* particle_rewards) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(seq);
    float* const outs[8] = {state_mean, state_std, reward_mean, reward_std, particle_states, particle_rewards, nullptr, nullptr};
    bbmpc::traj_particles_host(*h->e, states, seq, batch, horizon, eps, false, 0, nullptr, outs);
    API_END
}

int bbmpc_predict_trajectory_quantiles_dev(bbmpc_handle h, const float* d_states, const float* d_seq, int32_t batch, int32_t horizon,
                                           const float* d_eps, float* d_state_mean, float* d_state_std, float* d_reward_mean,
                                           float* d_reward_std, float* d_particle_states, float* d_particle_rewards, int32_t num_levels,
                                           const int32_t* ranks, float* d_state_quantiles, float* d_reward_quantiles) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    CHECK_PTR(d_seq);
    h->e->predict_trajectory_quantiles_dev(d_states, d_seq, batch, horizon, d_eps, d_state_mean, d_state_std, d_reward_mean, d_reward_std,
                                           d_particle_states, d_particle_rewards, num_levels, ranks, d_state_quantiles, d_reward_quantiles);
    API_END
}

int bbmpc_predict_trajectory_quantiles(bbmpc_handle h, const float* states, const float* seq, int32_t batch, int32_t horizon, const float* eps,
                                       float* state_mean, float* state_std, float* reward_mean, float* reward_std, float* particle_states,
                                       float* particle_rewards, int32_t num_levels, const int32_t* ranks, float* state_quantiles,
                                       float* reward_quantiles) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(seq);
    float* const outs[8] = {state_mean, state_std, reward_mean, reward_std, particle_states, particle_rewards, state_quantiles, reward_quantiles};
    bbmpc::traj_particles_host(*h->e, states, seq, batch, horizon, eps, true, num_levels, ranks, outs);
    API_END
}

}  // extern "C"
