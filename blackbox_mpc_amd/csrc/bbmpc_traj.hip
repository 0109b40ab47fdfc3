// Open-loop trajectory prediction: DeterministicTrajectoryEvaluator.predict_next_state / evaluate_next_reward
// (trajectory_evaluators/deterministic.py:79-127) composed Hq times from each row's own start state, every state and
// reward kept -- bbmpc_predict_trajectories[_dev] -- and the squared-error reduction behind
// SystemDynamicsHandler.multistep_error.  Which form serves which handle:
//   built-in pendulum                      k_traj_pendulum (kernels_traj.hpp), one launch
//   learned MLP, built-in reward           k_traj_mlp (kernels_mlp_traj.hpp, launched from bbmpc_mlp.hip), one launch
//   HIP-source dynamics and / or reward    bbmpc_user_traj (rtc.hpp), compiled on the handle's first prediction, one launch
//   on an analytic model (no callbacks)    (Engine::traj_user_fused, bbmpc_user.hip)
//   learned MLP, learned reward            k_traj_mlp for the states + k_reward_mlp_rows (kernels_reward_mlp.hpp), two launches
//   torch callbacks; learned model with    step by step: the handle's row kernels / callbacks Hq times
//   a transform or a HIP-source reward
// ... and plan readback (bbmpc_set_keep_plan / bbmpc_get_plan).
#include "abi_util.hpp"
#include "kernels_traj.hpp"

namespace bbmpc {

void Engine::traj_stepwise(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out) {
    const size_t ns = (size_t)batch * S;
    if (tj_x0.n < ns) { tj_x0.alloc(ns); tj_x1.alloc(ns); }
    if (d_rewards_out && tj_rew.n < (size_t)batch) tj_rew.alloc((size_t)batch);
    const float* cur = d_states;
    float* bufs[2] = {tj_x0.p, tj_x1.p};
    for (int t = 0; t < horizon; ++t) {
        float* nxt = bufs[t & 1];
        const float* acts = d_seq + (size_t)t * U;                    // row b's action of step t: horizon * U floats apart
        dynamics_rows(cur, acts, horizon * U, batch, nxt, t);
        if (d_rewards_out) {
            reward_rows(cur, nxt, acts, horizon * U, batch, tj_rew.p, 0, t);
            HIP_CHECK(hipMemcpy2DAsync(d_rewards_out + t, (size_t)horizon * 4, tj_rew.p, 4, 4, batch, hipMemcpyDeviceToDevice, stream));
        }
        if (d_states_out)
            HIP_CHECK(hipMemcpy2DAsync(d_states_out + (size_t)t * S, (size_t)horizon * S * 4, nxt, (size_t)S * 4, (size_t)S * 4, batch,
                                       hipMemcpyDeviceToDevice, stream));
        cur = nxt;
    }
}

void Engine::predict_trajectories_dev(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out,
                                      float* d_rewards_out) {
    REQUIRE(batch >= 1, BBMPC_E_INVALID, "batch must be >= 1");
    REQUIRE(horizon >= 1 && horizon <= 4096, BBMPC_E_INVALID, "horizon must be in [1, 4096]");
    REQUIRE(d_states_out || d_rewards_out, BBMPC_E_INVALID, "states_out and rewards_out are both null");
    if (cfg.dynamics == BBMPC_DYN_MLP && !has_xform() && !d_rewards_out) {
        // states only: a learned model's states do not depend on the reward, whatever kind the handle was created with
        traj_mlp(d_states, d_seq, batch, horizon, d_states_out, nullptr);
        return;
    }
    if (cfg.reward == BBMPC_REW_MLP) {                    // learned reward: the states, then one launch of the scorer's rows frame
        traj_mlp_reward_mlp(d_states, d_seq, batch, horizon, d_states_out, d_rewards_out);
        return;
    }
    if (user_path() && cfg.dynamics != BBMPC_DYN_MLP && !user_callbacks()) {
        traj_user_fused(d_states, d_seq, batch, horizon, d_states_out, d_rewards_out);
        return;
    }
    if (user_path()) {
        // per-agent runtime parameters: refuse a batch the agents do not divide before anything is launched
        if (cfg.reward == BBMPC_REW_USER && d_rewards_out && user_reward.nparams > 0 && !user_reward.cb) {
            (void)user_params_dev(1);                 // rtc.hpp USER_KIND_REWARD
            (void)rows_per_agent(1, batch);
        }
        if (cfg.dynamics == BBMPC_DYN_USER && user_dynamics.nparams > 0 && !user_dynamics.cb) {
            (void)user_params_dev(2);                 // USER_KIND_DYNAMICS
            (void)rows_per_agent(2, batch);
        }
        traj_stepwise(d_states, d_seq, batch, horizon, d_states_out, d_rewards_out);
        return;
    }
    if (cfg.dynamics == BBMPC_DYN_MLP) {
        traj_mlp(d_states, d_seq, batch, horizon, d_states_out, d_rewards_out);
        return;
    }
    const int fq1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER) ? 1 : 0;
    dim3 grid((batch + 63) / 64), block(64);
    if (fix(BBMPC_STRICT_MATH)) hipLaunchKernelGGL(k_traj_pendulum<false>, grid, block, 0, stream, d_states, d_seq, batch, horizon, fq1, d_states_out, d_rewards_out);
    else hipLaunchKernelGGL(k_traj_pendulum<true>, grid, block, 0, stream, d_states, d_seq, batch, horizon, fq1, d_states_out, d_rewards_out);
    HIP_CHECK(hipGetLastError());
}

void Engine::traj_sq_error_dev(const float* d_pred, const float* d_obs, int batch, int horizon, double* d_sumsq) {
    REQUIRE(batch >= 1, BBMPC_E_INVALID, "batch must be >= 1");
    REQUIRE(horizon >= 1 && horizon <= 4096, BBMPC_E_INVALID, "horizon must be in [1, 4096]");
    const int cols = horizon * S, blocks = (batch + TRAJ_ERR_ROWS - 1) / TRAJ_ERR_ROWS;
    REQUIRE(blocks <= 65535, BBMPC_E_UNSUPPORTED, "squared trajectory error: at most 65535 * 64 rows per call");
    if (tj_part.n < (size_t)blocks * cols) tj_part.alloc((size_t)blocks * cols);
    hipLaunchKernelGGL(k_traj_sq_error_partial, dim3((cols + 255) / 256, blocks), dim3(256), 0, stream, d_pred, d_obs, batch, cols, tj_part.p);
    hipLaunchKernelGGL(k_traj_sq_error_final, dim3((cols + 255) / 256), dim3(256), 0, stream, (const double*)tj_part.p, blocks, cols, d_sumsq);
    HIP_CHECK(hipGetLastError());
}

// The solution the last control step took its action from, [A,H,U]: the final distribution mean (CEM / PI2 / SPSA /
// CMA-ES, before PI2's / SPSA's shift), PSO's global best, RandomSearch's best particle -- read from the per-iteration
// record the switch keeps (the parity trace's buffers).
void Engine::get_plan(float* out) {
    REQUIRE(cfg.optimizer != BBMPC_OPT_NONE, BBMPC_E_STATE, "handle was created without an optimizer");
    REQUIRE(keep_plan && plan_ready, BBMPC_E_STATE,
            "plan readback is off: call bbmpc_set_keep_plan(h, 1) (Optimizer.keep_plan(True) / MPCPolicy.keep_plan(True)) BEFORE the "
            "control step whose plan is wanted");
    if (cfg.optimizer == BBMPC_OPT_RANDOM_SEARCH) {
        std::vector<int> best(A);
        std::vector<float> samples((size_t)N * A * HU);
        get_trace(0, BBMPC_TRACE_ELITES, best.data(), (int64_t)A * 4);
        get_trace(0, BBMPC_TRACE_SAMPLES, samples.data(), (int64_t)samples.size() * 4);
        for (int a = 0; a < A; ++a) {
            REQUIRE(best[a] >= 0 && best[a] < N, BBMPC_E_STATE, "plan readback: best particle index out of range");
            memcpy(out + (size_t)a * HU, samples.data() + ((size_t)best[a] * A + a) * HU, (size_t)HU * 4);
        }
        return;
    }
    get_trace(std::max(iters, 1) - 1, BBMPC_TRACE_MEAN, out, (int64_t)A * HU * 4);
}

}  // namespace bbmpc

extern "C" {

int bbmpc_set_keep_plan(bbmpc_handle h, int32_t enabled) {
    API_BEGIN
    CHECK_HANDLE(h);
    Engine& e = *h->e;
    e.invalidate_step_graph();
    if (enabled && e.auto_split > 1)
        throw HipError(BBMPC_E_UNSUPPORTED, "plan readback is per shard: not available for a population > 32768 (played as shards)");
    e.keep_plan = enabled != 0;
    e.plan_ready = false;
    e.trace_on = enabled != 0;           // the routing of bbmpc_set_trace: launch-per-iteration paths that keep every solution
    API_END
}

int bbmpc_get_plan(bbmpc_handle h, float* actions) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(actions);
    h->e->get_plan(actions);
    API_END
}

int bbmpc_predict_trajectories_dev(bbmpc_handle h, const float* d_states, const float* d_seq, int32_t batch, int32_t horizon,
                                   float* d_states_out, float* d_rewards_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    CHECK_PTR(d_seq);
    h->e->predict_trajectories_dev(d_states, d_seq, batch, horizon, d_states_out, d_rewards_out);
    API_END
}

int bbmpc_predict_trajectories(bbmpc_handle h, const float* states, const float* seq, int32_t batch, int32_t horizon,
                               float* states_out, float* rewards_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(seq);
    Engine& e = *h->e;
    if (batch < 1) throw HipError(BBMPC_E_INVALID, "batch must be >= 1");
    if (horizon < 1 || horizon > 4096) throw HipError(BBMPC_E_INVALID, "horizon must be in [1, 4096]");
    if (!states_out && !rewards_out) throw HipError(BBMPC_E_INVALID, "states_out and rewards_out are both null");
    HostStage st(e);
    const int s = st.in(states, (size_t)batch * e.S), q = st.in(seq, (size_t)batch * horizon * e.U);
    const int so = st.out(states_out, (size_t)batch * horizon * e.S), ro = st.out(rewards_out, (size_t)batch * horizon);
    st.upload();
    e.predict_trajectories_dev(st[s], st[q], batch, horizon, st[so], st[ro]);
    st.finish();
    API_END
}

int bbmpc_trajectory_sq_error_dev(bbmpc_handle h, const float* d_predicted, const float* d_observed, int32_t batch, int32_t horizon,
                                  double* d_sum_sq) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_predicted);
    CHECK_PTR(d_observed);
    CHECK_PTR(d_sum_sq);
    h->e->traj_sq_error_dev(d_predicted, d_observed, batch, horizon, d_sum_sq);
    API_END
}

}  // extern "C"
