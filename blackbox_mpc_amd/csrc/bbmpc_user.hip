// User-supplied reward / dynamics functions and target transforms: the Engine members that compile (hiprtc, rtc.hpp),
// load and launch them, the step-wise evaluator (kernels_user.hpp), and their C ABI entry points.  Nothing launched here
// draws random numbers (candidates come from the core's Engine::draw_candidates): no quantile-table upload for this unit.
#include "abi_util.hpp"
#include "rtc.hpp"
#include "traj_particle_args.hpp"

namespace bbmpc {

// The code object of one program; a compiler failure comes back as BBMPC_E_INVALID with the log.  `compiles`: the handle's
// counter (bbmpc_compile_stats), which counts failed attempts too; null for the compile-only checks.
static std::vector<char> compile_checked(int form, const UserProgram& d, int64_t* compiles = nullptr) {
    if (compiles) ++*compiles;
    try {
        return compile_program(form, d);
    } catch (const std::exception& ex) {
        throw HipError(BBMPC_E_INVALID, ex.what());
    }
}

// Replaces the module of `f`: callers compile first, so a source that fails to compile leaves the previous function in place.
static void load_program(UserFunction& f, int form, const std::vector<char>& code) {
    f.release();
    HIP_CHECK(hipModuleLoadData(&f.module, code.data()));
    HIP_CHECK(hipModuleGetFunction(&f.fn, f.module, program_kernel(form)));
    if (form == USER_KIND_REWARD) {
        HIP_CHECK(hipModuleGetFunction(&f.fn_traj, f.module, "bbmpc_user_reward_traj"));
        HIP_CHECK(hipModuleGetFunction(&f.fn_particles, f.module, "bbmpc_user_reward_particles"));
        HIP_CHECK(hipModuleGetFunction(&f.fn_traj_particles, f.module, "bbmpc_user_reward_traj_particles"));
    }
}

// one lane per row; the launch reads as many entries of args[] as the kernel has, so a classic one ignores the parameters at the end
void Engine::launch_rows(hipFunction_t fn, int batch, void** args) {
    HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)((batch + 255) / 256), 1, 1, 256, 1, 1, 0, stream, args, nullptr));
}

// what the handle's programs are built from right now
UserProgram Engine::user_program() const {
    UserProgram d;
    d.S = S; d.U = U;
    d.dyn_kind = cfg.dynamics; d.rew_kind = cfg.reward;
    d.reward_src = user_reward.source; d.dynamics_src = user_dynamics.source; d.xform_src = user_xform.source;
    d.rew_np = user_reward.nparams; d.dyn_np = user_dynamics.nparams;
    return d;
}

// the reward / dynamics side of the handle: its function, its runtime parameters, what the handle must be created with
UserFunction& Engine::user_fn(int kind) { return kind == USER_KIND_REWARD ? user_reward : user_dynamics; }
Engine::UserParams& Engine::user_pp(int kind) { return kind == USER_KIND_REWARD ? rew_params : dyn_params; }
void Engine::require_user_side(int kind) const {
    if (kind == USER_KIND_REWARD) REQUIRE(cfg.reward == BBMPC_REW_USER, BBMPC_E_STATE, "handle was not created with BBMPC_REW_USER");
    else REQUIRE(cfg.dynamics == BBMPC_DYN_USER, BBMPC_E_STATE, "handle was not created with BBMPC_DYN_USER");
}

void Engine::set_user_source(int kind, const char* src, int nparams) {
    REQUIRE(src && *src, BBMPC_E_INVALID, "empty HIP source");
    require_user_side(kind);
    UserProgram d = user_program();
    d.own_source(kind) = src;
    (kind == USER_KIND_REWARD ? d.rew_np : d.dyn_np) = nparams;
    const std::vector<char> code = compile_checked(kind, d, &rtc_compiles);
    HIP_CHECK(hipStreamSynchronize(stream));
    UserFunction& f = user_fn(kind);
    load_program(f, kind, code);
    f.source = src;
    f.nparams = nparams;
    user_pp(kind).set = false;       // a new source starts without parameters
    f.cb = nullptr; f.cb_user = nullptr;
    user_rollout_stale = true;
    user_traj_stale = true;
    user_xform_rollout_stale = true;
}

void Engine::set_user_callback(int kind, bbmpc_rows_callback fn, void* user) {
    require_user_side(kind);
    REQUIRE(!(fn && value_on()), BBMPC_E_UNSUPPORTED,
            "a callback plug-in beside a learned terminal value (bbmpc_set_terminal_value_mlp): the step-wise rollout has no terminal-value form");
    REQUIRE(!(fn && prior_on()), BBMPC_E_UNSUPPORTED,
            "a callback plug-in beside a policy prior (bbmpc_set_policy_prior_mlp): the step-wise rollout draws for itself");
    REQUIRE(!(fn && kind == USER_KIND_DYNAMICS && has_xform()), BBMPC_E_UNSUPPORTED,
            "a dynamics callback returns absolute next states: apply the inverse target transform inside it (clear the transform first)");
    HIP_CHECK(hipStreamSynchronize(stream));
    UserFunction& f = user_fn(kind);
    if (fn) { f.release(); f.source.clear(); f.nparams = 0; }
    f.cb = fn;
    f.cb_user = fn ? user : nullptr;
    user_rollout_stale = true;
    user_traj_stale = true;
    user_xform_rollout_stale = true;
}

// Runtime parameters of a parameterised reward / dynamics: count = P (shared by every agent) or A * P (per local agent).
// Only uploads, never compiles.  Resident and graph-replayed control steps never run a user path (use_fused*() wants
// built-in plug-ins, graph_ok wants !user_path()), so the copy only has to be ordered on the handle's stream ahead of the
// next launch: it goes there, after whatever still reads the old rows, and is waited for, so `data` may go on return.
void Engine::set_user_params(int kind, const float* data, int64_t count) {
    REQUIRE(kind == USER_KIND_REWARD || kind == USER_KIND_DYNAMICS, BBMPC_E_INVALID, "kind must be 1 (reward) or 2 (dynamics)");
    REQUIRE(user_fn(kind).nparams > 0, BBMPC_E_STATE,
            kind == USER_KIND_REWARD ? "user reward: no parameterised source set (bbmpc_set_reward_source_params)"
                                     : "user dynamics: no parameterised source set (bbmpc_set_dynamics_source_params)");
    const int64_t P = user_fn(kind).nparams;
    REQUIRE(count == P || count == (int64_t)A * P, BBMPC_E_INVALID,
            "runtime parameters: count must be num_params (shared) or num_agents * num_params (per agent)");
    REQUIRE(data, BBMPC_E_INVALID, "runtime parameters: null data");
    std::vector<float> rows((size_t)A * P);
    for (int a = 0; a < A; ++a) memcpy(rows.data() + (size_t)a * P, data + (count == P ? 0 : (size_t)a * P), (size_t)P * 4);
    UserParams& pp = user_pp(kind);
    if (pp.d.n < rows.size()) {
        HIP_CHECK(hipStreamSynchronize(stream));       // the old buffer may still be read
        pp.d.alloc(rows.size());
    }
    HIP_CHECK(hipMemcpyAsync(pp.d.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    pp.set = true;
    pp.per_agent = count != P;
}

// the device rows of a parameterised function (nullptr for a classic one); refuses to compute before they were set
const float* Engine::user_params_dev(int kind) {
    if (user_fn(kind).nparams == 0) return nullptr;
    REQUIRE(user_pp(kind).set, BBMPC_E_STATE, kind == USER_KIND_REWARD ? "user reward: runtime parameters not set (bbmpc_set_user_params)"
                                                                       : "user dynamics: runtime parameters not set (bbmpc_set_user_params)");
    return user_pp(kind).d.p;
}

const float* Engine::user_reward_params_dev() { return user_params_dev(USER_KIND_REWARD); }

// rows of one agent in a batch of rows (the evaluator's layout b = a * rows + n): per-agent parameters need a multiple of A
// rows; shared ones any batch (every row then reads agent 0's copy)
int Engine::rows_per_agent(int kind, int batch) {
    if (!user_pp(kind).per_agent) return batch;
    REQUIRE(batch % A == 0, BBMPC_E_INVALID,
            "per-agent runtime parameters: a call on B rows needs B to be a multiple of num_agents (B / A consecutive rows per agent)");
    return batch / A;
}

// Target transforms (rtc.hpp): the inverse one on a learned-model or BBMPC_DYN_USER handle replaces next = dev + state
// in every rollout, step and row call of the handle; src NULL / empty clears it.  The forward one only serves
// transform_rows (training targets).  Compiled here, so a compiler error comes back from this call.
void Engine::set_transform_source(int kind, const char* src) {
    const bool clear = !src || !*src;
    const bool inverse = kind == USER_KIND_INVERSE_TRANSFORM;
    if (inverse && !clear) {
        REQUIRE(!value_on(), BBMPC_E_UNSUPPORTED,
                "an inverse target transform beside a learned terminal value (bbmpc_set_terminal_value_mlp): the transform rollout has no "
                "terminal-value form");
        REQUIRE(!shaping_on(), BBMPC_E_UNSUPPORTED,
                "an inverse target transform beside return shaping (bbmpc_set_return_shaping): the transform rollout has no shaped form");
        REQUIRE(!prior_on(), BBMPC_E_UNSUPPORTED,
                "an inverse target transform beside a policy prior (bbmpc_set_policy_prior_mlp): the policy rollout's model step is "
                "next = dev + state");
        REQUIRE(cfg.reward != BBMPC_REW_MLP, BBMPC_E_UNSUPPORTED,
                "an inverse target transform beside a learned reward model (BBMPC_REW_MLP): the transform rollout has no learned-reward form");
        REQUIRE(cfg.dynamics == BBMPC_DYN_MLP || cfg.dynamics == BBMPC_DYN_USER, BBMPC_E_UNSUPPORTED,
                "an inverse target transform needs a learned-model (BBMPC_DYN_MLP) or BBMPC_DYN_USER handle; the built-in pendulum "
                "model keeps next = dev + state");
        REQUIRE(!user_dynamics.cb, BBMPC_E_UNSUPPORTED,
                "inverse target transform: this handle's dynamics is a callback, which returns absolute next states itself");
    }
    // a BBMPC_DYN_USER handle's dynamics rows program inlines the inverse transform: rebuilt with the new one
    const bool rebuild_dyn = inverse && cfg.dynamics == BBMPC_DYN_USER && !user_dynamics.source.empty();
    UserProgram d = user_program();
    d.xform_src = clear ? "" : src;
    std::vector<char> code, dyn_code;
    if (!clear) code = compile_checked(kind, d, &rtc_compiles);
    if (rebuild_dyn) dyn_code = compile_checked(USER_KIND_DYNAMICS, d, &rtc_compiles);
    HIP_CHECK(hipStreamSynchronize(stream));
    UserFunction& f = inverse ? user_xform : user_fwd_xform;
    f.release();
    f.source.clear();
    if (!clear) {
        load_program(f, kind, code);
        f.source = src;
    }
    if (rebuild_dyn) load_program(user_dynamics, USER_KIND_DYNAMICS, dyn_code);
    if (inverse) {
        user_rollout_stale = true;
    user_traj_stale = true;
        user_xform_rollout_stale = true;
        user_xform_rollout.release();
    }
}

// out = transform(d_a, d_b) on [batch] rows: inverse (cur, dev) -> next, forward (cur, next) -> target
void Engine::transform_rows(int kind, const float* d_a, const float* d_b, int batch, float* d_out) {
    const UserFunction& f = kind == USER_KIND_INVERSE_TRANSFORM ? user_xform : user_fwd_xform;
    REQUIRE(f.fn, BBMPC_E_STATE, kind == USER_KIND_INVERSE_TRANSFORM ? "no inverse target transform set (bbmpc_set_inverse_transform_source)"
                                                                    : "no target transform set (bbmpc_set_transform_source)");
    void* args[] = {&d_a, &d_b, &batch, &d_out};
    launch_rows(f.fn, batch, args);
}

// total (+)= the rewards a callback wrote for one batch of rows
__global__ void k_rows_accumulate(const float* __restrict__ r, int batch, float* __restrict__ total, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < batch) total[i] = accumulate ? total[i] + r[i] : r[i];
}

// next = process_output(state, dynamics(process_input(state, action)))  on [batch] rows   deterministic.py:79-103
void Engine::dynamics_rows(const float* d_states, const float* d_actions, int astride, int batch, float* d_next, int t) {
    if (cfg.dynamics == BBMPC_DYN_USER && user_dynamics.cb) {
        // the callback sees a dense [batch, U] block
        if (user_dynamics.cb(user_dynamics.cb_user, d_states, dense_actions(d_actions, astride, batch), nullptr, batch, d_next, (void*)stream) != 0)
            throw HipError(BBMPC_E_INVALID, "the dynamics callback reported an error");
        return;
    }
    if (cfg.dynamics == BBMPC_DYN_USER) {
        REQUIRE(user_dynamics.fn, BBMPC_E_STATE, "user dynamics: call bbmpc_set_dynamics_source (or bbmpc_set_dynamics_callback) before computing");
        const float* params = user_params_dev(USER_KIND_DYNAMICS);                // a parameterised function only
        int rpa = params ? rows_per_agent(USER_KIND_DYNAMICS, batch) : 0;
        void* args[] = {&d_states, &d_actions, &astride, &batch, &d_next, &params, &rpa, &t};
        launch_rows(user_dynamics.fn, batch, args);
        return;
    }
    if (cfg.dynamics == BBMPC_DYN_PENDULUM) {
        hipLaunchKernelGGL(k_step_pendulum, dim3((batch + 63) / 64), dim3(64), 0, stream, d_states, d_actions, astride, batch,
                           (int)fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER), d_next, (float*)nullptr);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (has_xform()) {                                                    // learned model + inverse target transform
        mlp_xform_rows(d_states, d_actions, astride, batch, d_next);
        return;
    }
    step_dev(d_states, d_actions, astride, batch, d_next, nullptr);        // learned model (its built-in reward kind is REW_NONE here)
}

// total (+)= reward_function(cur, actions, next) on [batch] rows   deterministic.py:65-66, 105-127
void Engine::reward_rows(const float* d_cur, const float* d_next, const float* d_actions, int astride, int batch, float* d_total,
                         int accumulate, int t) {
    if (cfg.reward == BBMPC_REW_MLP) {                                    // the rows frame of kernels_reward_mlp.hpp: one reward per row
        REQUIRE(!accumulate, BBMPC_E_INVALID, "internal: a learned reward is never scored step by step");
        RewMlpRowsArgs q;
        memset(&q, 0, sizeof(q));
        q.B = batch;
        q.cur = d_cur; q.cur_stride = S;
        q.act = d_actions; q.act_stride = astride;
        q.nxt = d_next; q.nxt_stride = S;
        q.out = d_total;
        reward_mlp_rows(q);
        return;
    }
    if (cfg.reward == BBMPC_REW_USER && user_reward.cb) {
        const float* acts_c = dense_actions(d_actions, astride, batch);
        if (u_cb_rew.n < (size_t)batch) u_cb_rew.alloc((size_t)batch);
        if (user_reward.cb(user_reward.cb_user, d_cur, acts_c, d_next, batch, u_cb_rew.p, (void*)stream) != 0)
            throw HipError(BBMPC_E_INVALID, "the reward callback reported an error");
        hipLaunchKernelGGL(k_rows_accumulate, dim3((batch + 255) / 256), dim3(256), 0, stream, u_cb_rew.p, batch, d_total, accumulate);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (cfg.reward == BBMPC_REW_USER) {
        REQUIRE(user_reward.fn, BBMPC_E_STATE, "user reward: call bbmpc_set_reward_source (or bbmpc_set_reward_callback) before computing");
        const float* params = user_params_dev(USER_KIND_REWARD);                  // a parameterised function only
        int rpa = params ? rows_per_agent(USER_KIND_REWARD, batch) : 0;
        void* args[] = {&d_cur, &d_next, &d_actions, &astride, &batch, &d_total, &accumulate, &params, &rpa, &t};
        launch_rows(user_reward.fn, batch, args);
        return;
    }
    hipLaunchKernelGGL(k_reward_rows_acc, dim3((batch + 255) / 256), dim3(256), 0, stream, d_cur, d_next, d_actions, astride, batch, S, U,
                       (int)cfg.reward, (int)fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER), d_total, accumulate);
    HIP_CHECK(hipGetLastError());
}

// DeterministicMLP.__call__ on already-processed rows (deterministic_mlp.py:27-51)
__global__ __launch_bounds__(TAIL_THREADS) void k_rows_mlp_raw(RowMlp net, const float* x_in, float* out) {
    __shared__ float x[192];
    __shared__ float bufA[TAIL_MAXW], bufB[TAIL_MAXW], part[(TAIL_THREADS / 64) * TAIL_MAXW];
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int K = net.m.dims[0], M = net.m.dims[net.m.n_layers];
    for (int i = tid; i < K; i += nthr) x[i] = x_in[(size_t)b * K + i];
    __syncthreads();
    const float* raw = row_mlp_forward(net, x, bufA, bufB, part, tid, nthr);
    for (int i = tid; i < M; i += nthr) out[(size_t)b * M + i] = raw[i];
}

void Engine::mlp_forward_rows(const float* d_x, int batch, float* d_out) {
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP && mlp_ready, BBMPC_E_STATE, "bbmpc_mlp_forward: needs a learned-dynamics handle with weights set");
    hipLaunchKernelGGL(k_rows_mlp_raw, dim3(batch), dim3(TAIL_THREADS), 0, stream, row_mlp(), d_x, d_out);
    HIP_CHECK(hipGetLastError());
}

// Learned model + inverse target transform on rows, the step-wise twin of bbmpc_mlp_xform_rollout and the one-step path
// (predict_next_state, the next state act() returns): process_input, the Dense stack (k_rows_mlp_raw, k_tail_mlp's
// per-row code), de-normalise, then the user's transform rows (system_dynamics_handler.py:97-161).
void Engine::mlp_xform_rows(const float* d_states, const float* d_actions, int astride, int batch, float* d_next) {
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    const float* acts_c = dense_actions(d_actions, astride, batch);
    if (u_xin.n < (size_t)batch * (S + U)) u_xin.alloc((size_t)batch * (S + U));
    if (u_xraw.n < (size_t)batch * S) u_xraw.alloc((size_t)batch * S);
    const float* stats = mlp.normalized ? d_stats.p : nullptr;
    hipLaunchKernelGGL(k_process_input, dim3((batch * (S + U) + 255) / 256), dim3(256), 0, stream, d_states, acts_c, batch, S, U, stats, u_xin.p);
    hipLaunchKernelGGL(k_rows_mlp_raw, dim3(batch), dim3(TAIL_THREADS), 0, stream, row_mlp(), (const float*)u_xin.p, u_xraw.p);
    if (stats) hipLaunchKernelGGL(k_denormalize_rows, dim3((batch * S + 255) / 256), dim3(256), 0, stream, batch, S, U, stats, u_xraw.p);
    HIP_CHECK(hipGetLastError());
    transform_rows(USER_KIND_INVERSE_TRANSFORM, d_states, u_xraw.p, batch, d_next);
}

// DeterministicTrajectoryEvaluator.__call__ one planning step at a time (kernels_user.hpp)
void Engine::rollout_stepwise(int mode, bool pen, RolloutArgs& ra) {
    const int n_pop = ra.n_pop, Hh = ra.H, HUh = ra.HU;
    const size_t B = (size_t)A * n_pop;
    if (u_rows.n < (size_t)Hh * B * U) u_rows.alloc((size_t)Hh * B * U);
    if (u_x0.n < B * S) { u_x0.alloc(B * S); u_x1.alloc(B * S); }
    if (u_total.n < B) { u_total.alloc(B); u_pen.alloc(B); }
    dim3 grid((n_pop + 255) / 256, A), block(256);
    draw_candidates(mode, ra);
    RowsArgs rw;
    memset(&rw, 0, sizeof(rw));
    rw.n_pop = n_pop; rw.A = A; rw.H = Hh; rw.U = U; rw.S = S; rw.HU = HUh; rw.Nst = ra.Nst;
    rw.from_ref = mode == SRC_REF ? 1 : 0;
    rw.pen = pen ? 1 : 0;
    rw.seq = ra.seq;
    rw.cand = mode == SRC_BUF ? ra.cand : ra.samples;
    rw.samples = (mode == SRC_BUF && pen) ? ra.samples : nullptr;       // the feasible candidates go back (PSO / SPSA / CMA-ES / PI2)
    if (mode == SRC_TRUNC && pen) rw.samples = ra.samples;
    rw.lo = ra.lo; rw.hi = ra.hi;
    rw.state = ra.state;
    rw.rows = u_rows.p; rw.x0 = u_x0.p; rw.penalty = u_pen.p;
    prof_begin();
    hipLaunchKernelGGL(k_rows_prepare, grid, block, 0, stream, rw);
    HIP_CHECK(hipGetLastError());
    float* cur = u_x0.p;
    float* nxt = u_x1.p;
    for (int t = 0; t < Hh; ++t) {
        const float* acts = u_rows.p + (size_t)t * B * U;
        dynamics_rows(cur, acts, U, (int)B, nxt, t);
        reward_rows(cur, nxt, acts, U, (int)B, u_total.p, t > 0 ? 1 : 0, t);
        std::swap(cur, nxt);
    }
    hipLaunchKernelGGL(k_rows_finish, grid, block, 0, stream, n_pop, A, ra.Nst, pen ? 1 : 0, u_total.p, u_pen.p, ra.rewards, ra.penalty_out);
    HIP_CHECK(hipGetLastError());
    prof_end();
}

// The fused form for analytic models: one lane per trajectory, user function(s) inlined next to the engine's own
// model / rewards (rtc.hpp k_rollout_text).  Compiled on first use, after both sources are known.
void Engine::rollout_user_fused(int mode, bool pen, RolloutArgs& ra) {
    if (user_rollout_stale || !user_rollout.fn) {
        if (cfg.reward == BBMPC_REW_USER) REQUIRE(user_reward.fn, BBMPC_E_STATE, "user reward: call bbmpc_set_reward_source before computing");
        if (cfg.dynamics == BBMPC_DYN_USER) REQUIRE(user_dynamics.fn, BBMPC_E_STATE, "user dynamics: call bbmpc_set_dynamics_source before computing");
        load_program(user_rollout, PROG_ROLLOUT, compile_checked(PROG_ROLLOUT, user_program(), &rtc_compiles));
        user_rollout_stale = false;
    }
    int n_pop = ra.n_pop, Aa = A, Hh = ra.H, Nst_ = ra.Nst;
    draw_candidates(mode, ra);
    int from_ref = mode == SRC_REF ? 1 : 0, ipen = pen ? 1 : 0, fq1 = (int)fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER);
    const float* state = ra.state;
    const float* seq = ra.seq;
    const float* cand = mode == SRC_BUF ? ra.cand : ra.samples;
    float* samples = (pen && mode != SRC_REF) ? ra.samples : nullptr;          // the feasible candidates go back
    const float* lo_ = ra.lo;
    const float* hi_ = ra.hi;
    float* rewards = ra.rewards;
    float* penalty_out = ra.penalty_out;
    // parameterised sides only (else null); a classic program's kernel has 15 arguments and the launch reads no more
    // entries of args[] than the kernel has
    const float* rew_p = user_params_dev(USER_KIND_REWARD);
    const float* dyn_p = user_params_dev(USER_KIND_DYNAMICS);
    void* args[] = {&n_pop, &Aa, &Hh, &Nst_, &from_ref, &ipen, &fq1, &state, &seq, &cand, &samples, &lo_, &hi_, &rewards, &penalty_out,
                    &rew_p, &dyn_p};
    // few trajectories -> one wave per workgroup (latency); many -> 256-thread workgroups
    const unsigned bs = ((long)n_pop * A <= 16384) ? 64 : 256;
    prof_begin();
    HIP_CHECK(hipModuleLaunchKernel(user_rollout.fn, (unsigned)((n_pop + bs - 1) / bs), (unsigned)A, 1, bs, 1, 1, 0, stream, args, nullptr));
    prof_end();
}

// bbmpc_predict_trajectories for analytic models with a HIP-source function on either side: rtc.hpp's bbmpc_user_traj, one
// launch for all Hq steps.  Compiled on the handle's first prediction after the sources changed (one hiprtc run), so a
// handle that never predicts compiles what it always did; parameter updates never recompile.
void Engine::traj_user_fused(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out) {
    if (cfg.reward == BBMPC_REW_USER) REQUIRE(user_reward.fn, BBMPC_E_STATE, "user reward: call bbmpc_set_reward_source before computing");
    if (cfg.dynamics == BBMPC_DYN_USER) REQUIRE(user_dynamics.fn, BBMPC_E_STATE, "user dynamics: call bbmpc_set_dynamics_source before computing");
    const float* rew_p = user_params_dev(USER_KIND_REWARD);
    const float* dyn_p = user_params_dev(USER_KIND_DYNAMICS);
    int rew_rpa = rew_p ? rows_per_agent(USER_KIND_REWARD, batch) : batch;      // (refuses B % A != 0 before anything is launched)
    int dyn_rpa = dyn_p ? rows_per_agent(USER_KIND_DYNAMICS, batch) : batch;
    if (user_traj_stale || !user_traj.fn) {
        load_program(user_traj, PROG_TRAJ, compile_checked(PROG_TRAJ, user_program(), &rtc_compiles));
        user_traj_stale = false;
    }
    int fq1 = (int)fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER);
    void* args[] = {&batch, &horizon, &fq1, &d_states, &d_seq, &d_states_out, &d_rewards_out, &rew_p, &dyn_p, &rew_rpa, &dyn_rpa};
    const unsigned bs = batch <= 16384 ? 64 : 256;
    HIP_CHECK(hipModuleLaunchKernel(user_traj.fn, (unsigned)((batch + bs - 1) / bs), 1, 1, bs, 1, 1, 0, stream, args, nullptr));
}

// Learned MLP + user reward: the whole-horizon MFMA rollout (16-particle tiles) records the state after every step,
// then ONE launch of the user's function scores every trajectory -- 2 launches instead of 2*H + 2.
void Engine::rollout_mlp_user_reward(int mode, bool pen, RolloutArgs& ra) {
    REQUIRE(user_reward.fn_traj, BBMPC_E_STATE, "user reward: call bbmpc_set_reward_source before computing");
    const size_t need = (size_t)ra.H * A * ra.Nst * S;
    if (u_traj.n < need) u_traj.alloc(need);
    launch_rollout_mlp(mode, pen, ra, false, nullptr, u_traj.p);          // reward kind REW_NONE: leaves -(penalty) in ra.rewards
    int n_pop = ra.n_pop, Aa = A, Hh = ra.H, Nst_ = ra.Nst, from_ref = mode == SRC_REF ? 1 : 0;
    const float* state = ra.state;
    const float* traj = u_traj.p;
    const float* seq = ra.seq;
    const float* cand = mode == SRC_BUF ? ra.cand : ra.samples;
    float* rewards = ra.rewards;
    if (mode != SRC_REF) REQUIRE(cand, BBMPC_E_STATE, "user reward over the learned model: no candidate buffer");
    const float* params = user_params_dev(USER_KIND_REWARD);                  // a parameterised reward only
    void* args[] = {&n_pop, &Aa, &Hh, &Nst_, &from_ref, &state, &traj, &seq, &cand, &rewards, &params};
    HIP_CHECK(hipModuleLaunchKernel(user_reward.fn_traj, (unsigned)((n_pop + 255) / 256), (unsigned)A, 1, 256, 1, 1, 0, stream, args, nullptr));
}

// A HIP-source reward over the learned model's particles.  What the path refuses when it computes;
// bbmpc_set_particles has let the handle through on BBMPC_DYN_MLP + BBMPC_REW_USER alone.
void Engine::require_particle_user_reward() const {
    REQUIRE(!user_reward.cb, BBMPC_E_UNSUPPORTED,
            "particles with a callback reward: the particle evaluator needs a HIP-source reward (bbmpc_set_reward_source)");
    REQUIRE(user_reward.fn_particles && user_reward.fn_traj_particles, BBMPC_E_STATE, "user reward: call bbmpc_set_reward_source before computing");
}

// prewards [B][P][Hq] from the particle states k_traj_mlp_particles_kind left in pa.pstates: one lane per (b, p, t)
void Engine::score_traj_particles_user(const TrajParticleArgs& pa) {
    int B = pa.B, P = pa.P, Hq = pa.Hq;
    const float* states = pa.states;
    const float* seq = pa.seq;
    const float* pstates = pa.pstates;
    float* prewards = pa.prewards;
    const float* params = user_params_dev(USER_KIND_REWARD);
    int rpa = params ? rows_per_agent(USER_KIND_REWARD, B) : B;
    void* args[] = {&B, &P, &Hq, &states, &seq, &pstates, &prewards, &params, &rpa};
    const long n = (long)B * P * Hq;
    HIP_CHECK(hipModuleLaunchKernel(user_reward.fn_traj_particles, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, stream, args, nullptr));
}

// The learned-model rollout with the inverse target transform (and a user reward, if any) inlined: kernels_mlp_xform.hpp,
// compiled through hiprtc on first use after the sources change.  Candidates of RandomSearch / CEM / PI2 are drawn into the
// sample buffer first, as for the other user-function rollouts.
void Engine::rollout_mlp_xform(int mode, bool pen, RolloutArgs& ra) {
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    if (cfg.reward == BBMPC_REW_USER) REQUIRE(user_reward.fn, BBMPC_E_STATE, "user reward: call bbmpc_set_reward_source before computing");
    const XformLds lay = xform_lds_layout(mlp.tiles, mlp.n_layers, ra.H, S, U, mlp_nw);
    const size_t lds = (size_t)lay.total * sizeof(float);
    REQUIRE(lds <= 159 * 1024, BBMPC_E_UNSUPPORTED,
            "learned-model rollout with an inverse target transform: a 16-particle tile's action block plus the activation / "
            "partial-sum buffers of this network do not fit one CU's LDS (shorten the horizon or narrow the network)");
    bool act_ext = false;
    for (int l = 0; l < mlp.n_layers; ++l) act_ext = act_ext || mlp.act[l] > BBMPC_ACT_SIGMOID;
    if (user_xform_rollout_stale || !user_xform_rollout.fn || act_ext != user_xform_rollout_ext) {
        UserProgram d = user_program();
        d.act_ext = act_ext;
        load_program(user_xform_rollout, PROG_MLP_XFORM_ROLLOUT, compile_checked(PROG_MLP_XFORM_ROLLOUT, d, &rtc_compiles));
        user_xform_rollout_stale = false;
        user_xform_rollout_ext = act_ext;
    }
    draw_candidates(mode, ra);
    XformArgs x;
    memset(&x, 0, sizeof(x));
    x.n_pop = ra.n_pop; x.A = A; x.H = ra.H; x.Nst = ra.Nst;
    x.from_ref = mode == SRC_REF ? 1 : 0;
    x.pen = pen ? 1 : 0;
    x.fix_q1 = (int)fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER);
    x.nw = mlp_nw;
    x.n_layers = mlp.n_layers;
    x.normalized = mlp.normalized;
    for (int l = 0; l <= mlp.n_layers; ++l) x.tiles[l] = mlp.tiles[l];
    for (int l = 0; l < mlp.n_layers; ++l) { x.act[l] = mlp.act[l]; x.wp4[l] = d_wpack4[l].p; x.bpack[l] = mlp.bpack[l]; }
    x.mean_s = mlp.mean_s; x.std_s = mlp.std_s; x.mean_a = mlp.mean_a; x.std_a = mlp.std_a; x.mean_t = mlp.mean_t; x.std_t = mlp.std_t;
    x.state = ra.state;
    x.seq = ra.seq;
    x.cand = mode == SRC_BUF ? ra.cand : ra.samples;
    x.samples = (pen && mode != SRC_REF) ? ra.samples : nullptr;          // the feasible candidates go back
    x.lo = ra.lo; x.hi = ra.hi;
    x.rewards = ra.rewards;
    x.penalty_out = ra.penalty_out;
    if (mode != SRC_REF) REQUIRE(x.cand, BBMPC_E_STATE, "learned-model transform rollout: no candidate buffer");
    const float* rew_p = user_params_dev(USER_KIND_REWARD);
    void* args[] = {&x, &rew_p};                                               // the second one only for a parameterised reward
    prof_begin();
    HIP_CHECK(hipModuleLaunchKernel(user_xform_rollout.fn, (unsigned)((ra.n_pop + XF_TP - 1) / XF_TP), (unsigned)A, 1, (unsigned)(mlp_nw * 64),
                                    1, 1, (unsigned)lds, stream, args, nullptr));
    prof_end();
}

}  // namespace bbmpc

using bbmpc::UserProgram;

static void check_num_params(int32_t num_params) {
    if (num_params < 1) throw HipError(BBMPC_E_INVALID, "num_params must be >= 1 (a source without parameters: bbmpc_set_*_source)");
    if (num_params > BBMPC_MAX_USER_PARAMS)
        throw HipError(BBMPC_E_UNSUPPORTED, "num_params > " + std::to_string(BBMPC_MAX_USER_PARAMS) + " floats per agent");
}

// what a compile-only check starts from (the limit is a handle's: per-row arrays live in registers)
static UserProgram checked_program(int32_t dim_s, int32_t dim_u) {
    if (dim_s < 1 || dim_u < 1 || dim_s > 256 || dim_u > 256) throw HipError(BBMPC_E_INVALID, "dim_s / dim_u must be in [1, 256]");
    UserProgram d;
    d.S = dim_s; d.U = dim_u;
    return d;
}

// bbmpc_set_*_source (num_params null) and bbmpc_set_*_source_params
static void set_source(bbmpc_handle h, int kind, const char* src, const int32_t* num_params) {
    h->e->invalidate_step_graph();
    CHECK_PTR(src);
    if (num_params) check_num_params(*num_params);
    h->e->set_user_source(kind, src, num_params ? *num_params : 0);
}

extern "C" {

int bbmpc_set_reward_source(bbmpc_handle h, const char* src) {
    API_BEGIN
    CHECK_HANDLE(h);
    set_source(h, bbmpc::USER_KIND_REWARD, src, nullptr);
    API_END
}

int bbmpc_set_dynamics_source(bbmpc_handle h, const char* src) {
    API_BEGIN
    CHECK_HANDLE(h);
    set_source(h, bbmpc::USER_KIND_DYNAMICS, src, nullptr);
    API_END
}

int bbmpc_set_reward_source_params(bbmpc_handle h, const char* src, int32_t num_params) {
    API_BEGIN
    CHECK_HANDLE(h);
    set_source(h, bbmpc::USER_KIND_REWARD, src, &num_params);
    API_END
}

int bbmpc_set_dynamics_source_params(bbmpc_handle h, const char* src, int32_t num_params) {
    API_BEGIN
    CHECK_HANDLE(h);
    set_source(h, bbmpc::USER_KIND_DYNAMICS, src, &num_params);
    API_END
}

int bbmpc_set_reward_callback(bbmpc_handle h, bbmpc_rows_callback fn, void* user) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    h->e->set_user_callback(bbmpc::USER_KIND_REWARD, fn, user);
    API_END
}

int bbmpc_set_dynamics_callback(bbmpc_handle h, bbmpc_rows_callback fn, void* user) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    h->e->set_user_callback(bbmpc::USER_KIND_DYNAMICS, fn, user);
    API_END
}

// no invalidate_step_graph(): a captured step never covers a user path (optimize_host's graph_ok wants !user_path())
int bbmpc_set_user_params(bbmpc_handle h, int32_t kind, const float* data, int64_t count) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_user_params(kind, data, count);
    API_END
}

int bbmpc_compile_stats(bbmpc_handle h, int64_t* compiles) {
    API_BEGIN
    CHECK_HANDLE(h);
    if (compiles) *compiles = h->e->rtc_compiles;
    API_END
}

// Every program a parameterised source takes part in, compiled (no GPU).  The partner a side lacks is a classic stub.
int bbmpc_check_user_params(const char* rew_src, int32_t rew_np, const char* dyn_src, int32_t dyn_np, int32_t dim_s, int32_t dim_u) {
    API_BEGIN
    if (!rew_src && !dyn_src) throw HipError(BBMPC_E_INVALID, "no source given");
    if (rew_src) check_num_params(rew_np);
    if (dyn_src) check_num_params(dyn_np);
    static const char* const k_stub_reward =
        "__device__ float bbmpc_user_reward(const float* c, const float* a, const float* n, int S, int U) { return -n[0] * n[0]; }\n";
    static const char* const k_stub_dynamics =
        "__device__ void bbmpc_user_dynamics(const float* x, float* d, int S, int U) { for (int i = 0; i < S; ++i) d[i] = 0.01f * x[i]; }\n";
    static const char* const k_stub_xform =
        "__device__ void bbmpc_user_inverse_transform_targets(const float* c, const float* d, float* n, int S) "
        "{ for (int i = 0; i < S; ++i) n[i] = c[i] + d[i]; }\n";
    UserProgram d = checked_program(dim_s, dim_u);                           // both sides the user's
    d.dyn_kind = BBMPC_DYN_USER; d.rew_kind = BBMPC_REW_USER;
    d.reward_src = rew_src ? rew_src : k_stub_reward; d.rew_np = rew_src ? rew_np : 0;
    d.dynamics_src = dyn_src ? dyn_src : k_stub_dynamics; d.dyn_np = dyn_src ? dyn_np : 0;
    UserProgram x = d, r = d, b = d;
    x.xform_src = k_stub_xform;                                              // ... with an inverse target transform
    r.dyn_kind = BBMPC_DYN_PENDULUM; r.dynamics_src.clear(); r.dyn_np = 0;   // the reward beside the built-in pendulum
    b.reward_src.clear(); b.rew_np = 0;                                      // the dynamics beside a built-in reward
    if (rew_src) {
        (void)bbmpc::compile_checked(bbmpc::USER_KIND_REWARD, d);            // rows + traj scorer
        (void)bbmpc::compile_checked(bbmpc::PROG_ROLLOUT, r);
        if (dim_s <= 64 && dim_s + dim_u <= 128) (void)bbmpc::compile_checked(bbmpc::PROG_MLP_XFORM_ROLLOUT, x);   // the learned model's limits
    }
    if (dyn_src) {
        (void)bbmpc::compile_checked(bbmpc::USER_KIND_DYNAMICS, d);
        (void)bbmpc::compile_checked(bbmpc::USER_KIND_DYNAMICS, x);
        for (int rk : {BBMPC_REW_PENDULUM, BBMPC_REW_CHEETAH}) {
            b.rew_kind = rk;
            (void)bbmpc::compile_checked(bbmpc::PROG_ROLLOUT, b);
        }
    }
    (void)bbmpc::compile_checked(bbmpc::PROG_ROLLOUT, d);
    (void)bbmpc::compile_checked(bbmpc::PROG_TRAJ, d);                       // trajectory prediction, both sides the user's
    if (rew_src) (void)bbmpc::compile_checked(bbmpc::PROG_TRAJ, r);
    if (dyn_src) (void)bbmpc::compile_checked(bbmpc::PROG_TRAJ, b);
    API_END
}

int bbmpc_check_user_source(int32_t kind, const char* src, int32_t dim_s, int32_t dim_u) {
    API_BEGIN
    CHECK_PTR(src);
    if (kind < bbmpc::USER_KIND_REWARD || kind > bbmpc::USER_KIND_TRANSFORM)
        throw HipError(BBMPC_E_INVALID, "kind must be 1 (reward), 2 (dynamics), 3 (inverse target transform) or 4 (target transform)");
    UserProgram d = checked_program(dim_s, dim_u);
    d.own_source(kind) = src;
    (void)bbmpc::compile_checked(kind, d);
    API_END
}

int bbmpc_check_user_rollout(int32_t dynamics, int32_t reward, const char* dyn_src, const char* rew_src, int32_t dim_s, int32_t dim_u) {
    API_BEGIN
    if (dynamics != BBMPC_DYN_PENDULUM && dynamics != BBMPC_DYN_USER) throw HipError(BBMPC_E_INVALID, "fused user rollouts exist for analytic dynamics (pendulum / user)");
    if (reward < BBMPC_REW_PENDULUM || reward > BBMPC_REW_USER) throw HipError(BBMPC_E_INVALID, "unknown reward kind");
    if ((dynamics == BBMPC_DYN_USER && !dyn_src) || (reward == BBMPC_REW_USER && !rew_src)) throw HipError(BBMPC_E_INVALID, "missing source");
    UserProgram d = checked_program(dim_s, dim_u);
    d.dyn_kind = dynamics; d.rew_kind = reward;
    if (reward == BBMPC_REW_USER) d.reward_src = rew_src;
    if (dynamics == BBMPC_DYN_USER) d.dynamics_src = dyn_src;
    (void)bbmpc::compile_checked(bbmpc::PROG_ROLLOUT, d);
    (void)bbmpc::compile_checked(bbmpc::PROG_TRAJ, d);                       // ... and its trajectory-prediction twin
    API_END
}

int bbmpc_set_inverse_transform_source(bbmpc_handle h, const char* src) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    h->e->set_transform_source(bbmpc::USER_KIND_INVERSE_TRANSFORM, src);
    API_END
}

int bbmpc_set_transform_source(bbmpc_handle h, const char* src) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    h->e->set_transform_source(bbmpc::USER_KIND_TRANSFORM, src);
    API_END
}

int bbmpc_transform_rows(bbmpc_handle h, int32_t kind, const float* a, const float* b, int32_t batch, float* out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(a);
    CHECK_PTR(b);
    CHECK_PTR(out);
    Engine& e = *h->e;
    if (kind != bbmpc::USER_KIND_INVERSE_TRANSFORM && kind != bbmpc::USER_KIND_TRANSFORM)
        throw HipError(BBMPC_E_INVALID, "kind must be 3 (inverse target transform) or 4 (target transform)");
    if (batch < 1) throw HipError(BBMPC_E_INVALID, "batch must be >= 1");
    const size_t n = (size_t)batch * e.S;
    HostStage st(e);
    const int da = st.in(a, n), db = st.in(b, n), dout = st.out(out, n);
    st.upload();
    e.transform_rows(kind, st[da], st[db], batch, st[dout]);
    st.finish();
    API_END
}

int bbmpc_check_xform_rollout(int32_t reward, const char* xform_src, const char* rew_src, int32_t dim_s, int32_t dim_u) {
    API_BEGIN
    CHECK_PTR(xform_src);
    if (reward < BBMPC_REW_PENDULUM || reward > BBMPC_REW_USER) throw HipError(BBMPC_E_INVALID, "unknown reward kind");
    if (reward == BBMPC_REW_USER && !rew_src) throw HipError(BBMPC_E_INVALID, "missing reward source");
    // the learned model's limits (bbmpc_set_mlp)
    if (dim_s < 1 || dim_u < 1 || dim_s > 64 || dim_s + dim_u > 128) throw HipError(BBMPC_E_UNSUPPORTED, "dim_s <= 64 and dim_s + dim_u <= 128");
    UserProgram d = checked_program(dim_s, dim_u);
    d.rew_kind = reward;
    d.xform_src = xform_src;
    if (reward == BBMPC_REW_USER) d.reward_src = rew_src;
    (void)bbmpc::compile_checked(bbmpc::PROG_MLP_XFORM_ROLLOUT, d);
    API_END
}

int bbmpc_mlp_forward(bbmpc_handle h, const float* x, int32_t batch, float* out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(x);
    CHECK_PTR(out);
    Engine& e = *h->e;
    if (batch < 1) throw HipError(BBMPC_E_INVALID, "batch must be >= 1");
    if (e.cfg.dynamics != BBMPC_DYN_MLP || !e.mlp_ready) throw HipError(BBMPC_E_STATE, "bbmpc_mlp_forward: needs a learned-dynamics handle with weights set");
    HostStage st(e);
    const int dx = st.in(x, (size_t)batch * e.mlp.dims[0]), dout = st.out(out, (size_t)batch * e.mlp.dims[e.mlp.n_layers]);
    st.upload();
    e.mlp_forward_rows(st[dx], batch, st[dout]);
    st.finish();
    API_END
}

}  // extern "C"
