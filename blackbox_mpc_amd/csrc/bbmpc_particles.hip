// Particle trajectory evaluator (bbmpc_set_particles, bbmpc_set_particle_risk, bbmpc_evaluate_particles;
// kernels_particles.hpp): the switch, the scoring rule, the process-noise buffer, the launch sequence  candidates -> noisy rollouts -> aggregate  that Engine::launch_rollout takes
// while the switch is on, and the ABI.  The learned model's rollout kernel is launched from bbmpc_mlp.hip.
#include <cmath>

#include "abi_util.hpp"
#include "kernels_particles.hpp"
#include "kernels_particle_constraint.hpp"

namespace bbmpc {

void Engine::set_particles(int num_particles, const float* sigma, float kappa) {
    REQUIRE(num_particles >= 0 && num_particles <= PARTICLES_MAX, BBMPC_E_INVALID, "num_particles must be in [0, 64]");
    invalidate_step_graph();
    if (num_particles == 0) {
        part_P = 0;
        pnoise_valid = false;
        if (cc_on) {                                                   // the chance constraint lives on the particles
            HIP_CHECK(hipStreamSynchronize(stream));
            cc_on = false;
            cc_last_npop = cc_last_Nst = cc_last_RS = cc_last_P = 0;
        }
        return;
    }
    REQUIRE(sigma != nullptr, BBMPC_E_INVALID, "null pointer argument: sigma");
    for (int s = 0; s < S; ++s)
        REQUIRE(std::isfinite(sigma[s]) && sigma[s] >= 0.0f, BBMPC_E_INVALID, "process noise sigma must be finite and >= 0");
    REQUIRE(std::isfinite(kappa), BBMPC_E_INVALID, "risk_kappa must be finite");
    REQUIRE(!grad_on(), BBMPC_E_UNSUPPORTED,
            "particles beside gradient refinement (bbmpc_set_grad_refine): the gradient is that of one noise-free rollout; switch it off "
            "first (steps = 0)");
    REQUIRE(cfg.reward != BBMPC_REW_MLP, BBMPC_E_UNSUPPORTED,
            "particles with a learned reward model (BBMPC_REW_MLP): the particle evaluator scores built-in and HIP-source rewards only");
    REQUIRE(!value_on(), BBMPC_E_UNSUPPORTED,
            "particles with a learned terminal value (bbmpc_set_terminal_value_mlp): the particle evaluator has no terminal term; remove "
            "the value network first (n_layers = 0)");
    REQUIRE(!shaping_on(), BBMPC_E_UNSUPPORTED,
            "particles with return shaping on (bbmpc_set_return_shaping): the particle evaluator has no shaped form; switch shaping "
            "off first (discount = 1, no bounds)");
    // a HIP-source reward scores the learned model's particles; the analytic pendulum keeps its built-in rewards
    REQUIRE((cfg.reward != BBMPC_REW_USER || cfg.dynamics == BBMPC_DYN_MLP) && cfg.dynamics != BBMPC_DYN_USER, BBMPC_E_UNSUPPORTED,
            "particles with HIP-source or callback dynamics, or with a user reward beside the built-in pendulum model: a user reward "
            "scores the noisy rollouts of a learned model (BBMPC_DYN_MLP) only");
    REQUIRE(!has_xform(), BBMPC_E_UNSUPPORTED, "particles with an inverse target transform: the noise is added to next = dev + state");
    REQUIRE(!pop_sharded() && cfg.population_global <= N, BBMPC_E_UNSUPPORTED,
            "particles with a sharded population: the shards would have to exchange per-particle returns");
    REQUIRE((long)N * num_particles <= 32768, BBMPC_E_UNSUPPORTED, "particles: population_size * num_particles must not exceed 32768");
    REQUIRE(ens_E == 0 || num_particles % ens_E == 0, BBMPC_E_INVALID,
            "particles: num_particles = " + std::to_string(num_particles) + " is no multiple of the model ensemble's num_members = " +
                std::to_string(ens_E) + " (the members must carry equal weight in the mean)");
    REQUIRE(part_risk != BBMPC_RISK_CVAR || part_tail <= num_particles, BBMPC_E_INVALID,
            "particles: num_particles = " + std::to_string(num_particles) + " is below the CVaR tail_count = " + std::to_string(part_tail) +
                " of bbmpc_set_particle_risk");
    HIP_CHECK(hipStreamSynchronize(stream));
    if (num_particles != part_P) inj.erase(BBMPC_NOISE_PROCESS);       // (its layout depends on P)
    if (d_psigma.n < (size_t)S) d_psigma.alloc((size_t)S);
    HIP_CHECK(hipMemcpy(d_psigma.p, sigma, (size_t)S * 4, hipMemcpyHostToDevice));
    const size_t ne = (size_t)A * num_particles * H * S;
    if (d_pnoise.n < ne) d_pnoise.alloc(ne);
    part_P = num_particles;
    part_kappa = kappa;
    pnoise_valid = false;
}

void Engine::set_particle_risk(int kind, int tail_count) {
    REQUIRE(kind == BBMPC_RISK_MEAN_STD || kind == BBMPC_RISK_CVAR, BBMPC_E_INVALID, "particle risk: unknown kind " + std::to_string(kind));
    if (kind == BBMPC_RISK_MEAN_STD) {
        REQUIRE(tail_count == 0, BBMPC_E_INVALID, "particle risk: tail_count must be 0 with BBMPC_RISK_MEAN_STD");
    } else {
        // (particles off: the rule against P is bbmpc_set_particles' to enforce)
        const int pmax = part_P > 0 ? part_P : PARTICLES_MAX;
        REQUIRE(tail_count >= 1 && tail_count <= pmax, BBMPC_E_INVALID,
                "particle risk: CVaR tail_count = " + std::to_string(tail_count) + " must be in [1, num_particles = " + std::to_string(pmax) + "]");
    }
    invalidate_step_graph();
    part_risk = kind;
    part_tail = tail_count;
}

// eps [A][P][H][S] of (control step, iteration): the injected tensor, or the handle's own draws, generated once per
// (step, iteration) however many rollouts share them (SPSA's plus and minus candidates do).
const float* Engine::process_noise(uint32_t step, uint32_t iter) {
    const size_t ne = (size_t)A * part_P * H * S;
    if (const float* in = injected(BBMPC_NOISE_PROCESS)) return in + ne * std::min<size_t>(iter, (size_t)std::max(iters, 1) - 1);
    if (pnoise_valid && pnoise_step == step && pnoise_iter == iter) return d_pnoise.p;
    RngKey kk = key(step);
    kk.q_per_agent = (uint32_t)((H * S + 3) / 4);
    kk.step_src = nullptr;
    const int blocks = A * part_P * (int)kk.q_per_agent;
    hipLaunchKernelGGL(k_gen_process_noise, dim3((blocks + 255) / 256), dim3(256), 0, stream, kk, iter, A, part_P, H * S, cfg.agent_offset,
                       d_pnoise.p);
    HIP_CHECK(hipGetLastError());
    pnoise_valid = true; pnoise_step = step; pnoise_iter = iter;
    return d_pnoise.p;
}

void Engine::dump_process_noise(int control_step, int iteration, float* out, int64_t count) {
    REQUIRE(particles_on(), BBMPC_E_STATE, "dump_noise: process noise needs bbmpc_set_particles first");
    const int64_t total = (int64_t)A * part_P * H * S;
    REQUIRE(count == total, BBMPC_E_INVALID, "dump_noise: process noise is [A, P, H, S]");
    RngKey kk = key((uint32_t)control_step);
    kk.q_per_agent = (uint32_t)((H * S + 3) / 4);
    kk.step_src = nullptr;
    const int blocks = A * part_P * (int)kk.q_per_agent;
    stage_read_back(*this, out, (size_t)total, [&](float* d) {
        hipLaunchKernelGGL(k_gen_process_noise, dim3((blocks + 255) / 256), dim3(256), 0, stream, kk, (uint32_t)iteration, A, part_P, H * S,
                           cfg.agent_offset, d);
    });
}

// launch_rollout with particles on: the candidates into the sample buffer (as the user-function paths draw them), the
// noisy rollouts of every (candidate, particle) row, the aggregate into ra.rewards.  d_returns: where the per-particle
// returns [A][returns_stride] go (null: the handle's own buffer).
void Engine::rollout_particles(int mode, bool pen, RolloutArgs& ra, float* d_returns, int returns_stride) {
    const bool user_rew = particle_user_reward();          // a HIP-source reward over the learned model: TRAJ rollout + scorer
    REQUIRE(!user_path() || user_rew, BBMPC_E_UNSUPPORTED, "particles with user-supplied dynamics or an inverse target transform");
    const int P = part_P;
    const bool boxed = cc_on && cfg.dynamics == BBMPC_DYN_MLP;      // bbmpc_set_chance_constraint: the TRAJ form whatever the reward
    if (user_rew) {                                        // refused before anything is allocated, drawn or launched
        require_particle_user_reward();
        (void)user_reward_params_dev();                    // (declared but not set: BBMPC_E_STATE)
    }
    if (user_rew || boxed) require_particle_traj_fits(d_returns ? returns_stride : (long)ra.Nst * P);
    if (!d_returns) {
        returns_stride = ra.Nst * P;
        if (d_preturns.n < (size_t)A * returns_stride) d_preturns.alloc((size_t)A * returns_stride);
        d_returns = d_preturns.p;
    }
    REQUIRE(returns_stride >= ra.n_pop * P, BBMPC_E_INVALID, "internal: particle returns stride");
    draw_candidates(mode, ra);
    ParticleArgs q;
    memset(&q, 0, sizeof(q));
    q.n_pop = ra.n_pop; q.P = P; q.A = A; q.H = ra.H; q.U = U; q.S = S; q.HU = ra.HU; q.Nst = ra.Nst; q.RS = returns_stride;
    q.from_ref = mode == SRC_REF ? 1 : 0;
    q.pen = pen ? 1 : 0;
    q.fix_q1 = ra.fix_q1; q.reward_kind = ra.reward_kind;
    q.state = ra.state; q.seq = ra.seq;
    q.cand = mode == SRC_BUF ? ra.cand : ra.samples;
    q.lo = ra.lo; q.hi = ra.hi;
    q.sigma = d_psigma.p;
    q.pnoise = process_noise(ra.key.step, ra.iter);
    q.returns = d_returns;
    q.samples = (pen && mode != SRC_REF) ? ra.samples : nullptr;          // the feasible candidates go back
    q.rewards = ra.rewards;
    q.penalty_out = ra.penalty_out;
    REQUIRE(ra.H == H, BBMPC_E_INVALID, "internal: particle rollout horizon");
    if (user_rew || boxed) {
        const size_t need = (size_t)ra.H * A * S * returns_stride;
        if (d_ptraj.n < need) d_ptraj.alloc(need);
        q.traj = d_ptraj.p;
    }
    if (boxed) {
        if (d_cc_first.n < (size_t)A * returns_stride) d_cc_first.alloc((size_t)A * returns_stride);
        if (d_cc_viol.n < (size_t)A * ra.Nst) d_cc_viol.alloc((size_t)A * ra.Nst);
    }
    const long rows = (long)ra.n_pop * P;
    ParticleConstraintArgs cq;
    memset(&cq, 0, sizeof(cq));
    dominant_inst[0] = 0;
    prof_begin();
    if (cfg.dynamics == BBMPC_DYN_MLP) {
        dominant_kernel = lv_heads > 0 ? "k_rollout_mlp_particles_gauss" : ens_E > 0 ? "k_rollout_mlp_particles_ens" : "k_rollout_mlp_particles";
        launch_rollout_mlp_particles(q);
        if (user_rew) score_particles_user(q);             // inside the profiled span, under the kind's name
        if (boxed) {                                       // the box scan; a built-in reward's returns come from it too
            cq.p = q;
            cq.box = d_cc_box.p; cq.first = d_cc_first.p; cq.viol = d_cc_viol.p;
            cq.delta = cc_delta; cq.lambda = cc_lambda;
            const dim3 sgrid((unsigned)((rows + PCS_LANES - 1) / PCS_LANES), A), sblock(PCS_LANES);
            if (user_rew) hipLaunchKernelGGL(k_particle_box_scan<false>, sgrid, sblock, 0, stream, cq);
            else hipLaunchKernelGGL(k_particle_box_scan<true>, sgrid, sblock, (size_t)particle_box_scan_lds_floats(S, U) * sizeof(float), stream, cq);
            HIP_CHECK(hipGetLastError());
        }
    } else {
        dominant_kernel = "k_rollout_pendulum_particles";
        // few rows -> one wave per workgroup so every wave gets its own SIMD; many -> 256-thread workgroups
        const int bs = (rows * A <= 16384) ? 64 : 256;
        hipLaunchKernelGGL(k_rollout_pendulum_particles, dim3((unsigned)((rows + bs - 1) / bs), A), dim3(bs), 0, stream, q);
        HIP_CHECK(hipGetLastError());
    }
    if (!boxed) prof_end();
    if (part_risk == BBMPC_RISK_CVAR)
        hipLaunchKernelGGL(k_particle_aggregate_cvar, dim3((ra.n_pop + CVAR_WAVES - 1) / CVAR_WAVES, A), dim3(CVAR_WAVES * 64), 0, stream, q,
                           part_tail);
    else
        hipLaunchKernelGGL(k_particle_aggregate, dim3((ra.n_pop + 255) / 256, A), dim3(256), 0, stream, q, part_kappa);
    HIP_CHECK(hipGetLastError());
    if (boxed) {                                           // behind the unchanged aggregate; the profiled span closes behind it
        hipLaunchKernelGGL(k_particle_constraint_apply, dim3((ra.n_pop + 255) / 256, A), dim3(256), 0, stream, cq);
        HIP_CHECK(hipGetLastError());
        prof_end();
        cc_last_npop = ra.n_pop; cc_last_Nst = ra.Nst; cc_last_RS = returns_stride; cc_last_P = P;
    }
}

// returns [A][RS] from the states the TRAJ rollout left in pa.traj: one lane per (candidate, particle) row, grid.y = agent
void Engine::score_particles_user(const ParticleArgs& pa) {
    int n_pop = pa.n_pop, P = pa.P, Aa = A, Hh = pa.H, Nst_ = pa.Nst, RS = pa.RS, from_ref = pa.from_ref, ipen = pa.pen;
    const float* state = pa.state;
    const float* traj = pa.traj;
    const float* seq = pa.seq;
    const float* cand = pa.cand;
    const float* lo_ = pa.lo;
    const float* hi_ = pa.hi;
    float* returns = pa.returns;
    if (!from_ref) REQUIRE(cand, BBMPC_E_STATE, "user reward over the learned model's particles: no candidate buffer");
    const float* params = user_reward_params_dev();                  // a parameterised reward only
    void* args[] = {&n_pop, &P, &Aa, &Hh, &Nst_, &RS, &from_ref, &ipen, &state, &traj, &seq, &cand, &lo_, &hi_, &returns, &params};
    const long rows = (long)n_pop * P;
    const unsigned bs = (rows * A <= 16384) ? 64 : 256;                       // as k_rollout_pendulum_particles sizes its workgroups
    HIP_CHECK(hipModuleLaunchKernel(user_reward.fn_particles, (unsigned)((rows + bs - 1) / bs), (unsigned)A, 1, bs, 1, 1, 0, stream, args, nullptr));
}


// the TRAJ rollout's buffer [H][A][S][RS] is addressed with 32-bit offsets
void Engine::require_particle_traj_fits(long returns_stride) const {
    REQUIRE((long)H * A * S * returns_stride < (1L << 31), BBMPC_E_UNSUPPORTED,
            "particles with a HIP-source reward or a chance constraint: horizon * num_agents * dim_s * (candidates * num_particles) reaches 2^31 trajectory elements");
}

// Chance constraint.  Everything is checked before the handle is touched, so a refusal leaves it as
// it was.  lo == hi == NULL removes it: the handle's launches and scores are then what they were before it was installed.
void Engine::set_chance_constraint(const float* lo, const float* hi, float max_violation, float weight) {
    REQUIRE((lo == nullptr) == (hi == nullptr), BBMPC_E_INVALID, "chance constraint: lo and hi must both be given, or both be NULL (remove)");
    if (!lo) {
        if (!cc_on) return;
        invalidate_step_graph();
        HIP_CHECK(hipStreamSynchronize(stream));
        cc_on = false;
        cc_last_npop = cc_last_Nst = cc_last_RS = cc_last_P = 0;
        return;
    }
    for (int i = 0; i < S; ++i) {
        REQUIRE(lo[i] == lo[i] && hi[i] == hi[i], BBMPC_E_INVALID,
                "chance constraint: state bound " + std::to_string(i) + " is NaN (use -inf / +inf for unbounded)");
        REQUIRE(lo[i] <= hi[i], BBMPC_E_INVALID, "chance constraint: lo[" + std::to_string(i) + "] exceeds hi[" + std::to_string(i) + "]");
    }
    REQUIRE(std::isfinite(max_violation) && max_violation >= 0.0f && max_violation < 1.0f, BBMPC_E_INVALID,
            "chance constraint: max_violation must be in [0, 1)");
    REQUIRE(std::isfinite(weight) && weight >= 0.0f, BBMPC_E_INVALID, "chance constraint: weight must be finite and >= 0");
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP, BBMPC_E_UNSUPPORTED,
            "chance constraint: the box is tested on the recorded particle rollouts of a learned model: the handle needs BBMPC_DYN_MLP, not "
            "analytic or user dynamics");
    REQUIRE(particles_on(), BBMPC_E_STATE, "chance constraint: particles are off: call bbmpc_set_particles first");
    REQUIRE(!(cfg.reward == BBMPC_REW_USER && user_reward.cb), BBMPC_E_UNSUPPORTED,
            "chance constraint with a callback reward: the particle evaluator needs a built-in or HIP-source reward (bbmpc_set_reward_source)");
    std::vector<float> box((size_t)2 * S);
    for (int i = 0; i < S; ++i) {
        box[i] = lo[i];
        box[S + i] = hi[i];
    }
    invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(stream));               // (nothing in flight reads the box that is replaced)
    cc_on = false;
    if (d_cc_box.n < box.size()) d_cc_box.alloc(box.size());
    HIP_CHECK(hipMemcpy(d_cc_box.p, box.data(), box.size() * 4, hipMemcpyHostToDevice));
    cc_delta = max_violation;
    cc_lambda = weight;
    cc_last_npop = cc_last_Nst = cc_last_RS = cc_last_P = 0;
    cc_on = true;
}

// v [n_pop, A] and first [n_pop, P, A] of the most recent particle rollout, in the layouts of bbmpc_evaluate_particles
void Engine::constraint_violations(int n_pop, float* prob_out, int32_t* first_out) {
    REQUIRE(constraint_on(), BBMPC_E_STATE, "constraint violations: no chance constraint is installed (bbmpc_set_chance_constraint)");
    REQUIRE(cc_last_npop > 0, BBMPC_E_STATE, "constraint violations: nothing has been rolled out since the chance constraint was installed");
    REQUIRE(prob_out != nullptr, BBMPC_E_INVALID, "null pointer argument: prob_out");
    REQUIRE(n_pop == cc_last_npop, BBMPC_E_INVALID,
            "constraint violations: n_pop must be the candidates of the most recent rollout = " + std::to_string(cc_last_npop));
    const int P = cc_last_P;
    std::vector<float> v((size_t)A * n_pop);
    std::vector<int32_t> f(first_out ? (size_t)A * n_pop * P : 0);
    HIP_CHECK(hipMemcpy2DAsync(v.data(), (size_t)n_pop * 4, d_cc_viol.p, (size_t)cc_last_Nst * 4, (size_t)n_pop * 4, A, hipMemcpyDeviceToHost, stream));
    if (first_out)
        HIP_CHECK(hipMemcpy2DAsync(f.data(), (size_t)n_pop * P * 4, d_cc_first.p, (size_t)cc_last_RS * 4, (size_t)n_pop * P * 4, A,
                                   hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (int a = 0; a < A; ++a)
        for (int n = 0; n < n_pop; ++n) {
            prob_out[(size_t)n * A + a] = v[(size_t)a * n_pop + n];
            if (first_out)
                for (int p = 0; p < P; ++p) first_out[((size_t)n * P + p) * A + a] = f[((size_t)a * n_pop + n) * P + p];
        }
}

// bbmpc_get_state / bbmpc_set_state names of the constraint's tests: the buffers of the most recent rollout as they lie in
// HBM, padding included ("constraint_first_raw" carries int32 bits).  true: the name was one of them.
bool Engine::constraint_raw_state(const std::string& name, float* out, const float* in, int64_t count) {
    if (name == "constraint_shape") {                     // (n_pop, Nst, RS, P) of the most recent constrained rollout; zeros: none
        REQUIRE(out && count == 4, BBMPC_E_INVALID, "constraint_shape has four elements and cannot be set");
        out[0] = (float)cc_last_npop; out[1] = (float)cc_last_Nst; out[2] = (float)cc_last_RS; out[3] = (float)cc_last_P;
        return true;
    }
    void* buf = nullptr;
    size_t n = 0;
    if (name == "constraint_first_raw") { buf = d_cc_first.p; n = (size_t)A * cc_last_RS; }
    else if (name == "constraint_viol_raw") { buf = d_cc_viol.p; n = (size_t)A * cc_last_Nst; }
    else if (name == "particle_returns_raw") { buf = d_preturns.p; n = (size_t)A * cc_last_RS; }
    else return false;
    REQUIRE(cc_last_npop > 0 && buf, BBMPC_E_STATE, name + ": nothing has been rolled out under a chance constraint");
    REQUIRE(count == (int64_t)n, BBMPC_E_INVALID, name + " has num_agents * stride elements (bbmpc_get_state \"constraint_shape\")");
    if (out) HIP_CHECK(hipMemcpy(out, buf, n * 4, hipMemcpyDeviceToHost));
    else HIP_CHECK(hipMemcpy(buf, in, n * 4, hipMemcpyHostToDevice));
    return true;
}

// scores [n_pop, A] and (optional) returns [n_pop, P, A] in the reference's layouts, from the caller's sequences
void Engine::evaluate_particles_dev(const float* d_state_in, const float* d_seq, int n_pop, float* d_scores, float* d_ret_out) {
    REQUIRE(particles_on(), BBMPC_E_STATE, "particles are off: call bbmpc_set_particles first");
    REQUIRE(n_pop >= 1, BBMPC_E_INVALID, "n_pop must be >= 1");
    REQUIRE((long)n_pop * part_P <= (1L << 24), BBMPC_E_UNSUPPORTED, "particles: n_pop * num_particles must not exceed 2^24 per call");
    const int P = part_P;
    const int st = ((n_pop + 63) / 64) * 64;
    if (particle_user_reward() || constraint_on()) require_particle_traj_fits((long)st * P);
    if (d_eval_rew.n < (size_t)A * st) d_eval_rew.alloc((size_t)A * st);
    RolloutArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.n_pop = n_pop; ra.A = A; ra.H = H; ra.U = U; ra.S = S; ra.HU = HU; ra.Nst = st;
    ra.agent_offset = cfg.agent_offset;
    ra.fix_q1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER);
    ra.reward_kind = builtin_reward_kind();
    ra.state = d_state_in;
    ra.seq = d_seq;
    ra.lo = d_lo.p; ra.hi = d_hi.p;
    ra.rewards = d_eval_rew.p;
    ra.key = key(step_counter);                   // the handle's current control step, iteration 0
    ra.iter = 0;
    rollout_particles(SRC_REF, false, ra, nullptr, 0);
    for (int a = 0; a < A; ++a) {
        // [A][st] -> [n_pop][A] and [A][st * P] (row n * P + p) -> [n_pop][P][A]: strided copies per agent (A is small)
        HIP_CHECK(hipMemcpy2DAsync(d_scores + a, (size_t)A * 4, d_eval_rew.p + (size_t)a * st, 4, 4, n_pop, hipMemcpyDeviceToDevice, stream));
        if (d_ret_out)
            HIP_CHECK(hipMemcpy2DAsync(d_ret_out + a, (size_t)A * 4, d_preturns.p + (size_t)a * st * P, 4, 4, (size_t)n_pop * P,
                                       hipMemcpyDeviceToDevice, stream));
    }
}

}  // namespace bbmpc

extern "C" {

int bbmpc_set_particles(bbmpc_handle h, int32_t num_particles, const float* sigma, float risk_kappa) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_particles(num_particles, sigma, risk_kappa);
    API_END
}

int bbmpc_set_particle_risk(bbmpc_handle h, int32_t kind, int32_t tail_count) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_particle_risk(kind, tail_count);
    API_END
}

int bbmpc_set_chance_constraint(bbmpc_handle h, const float* lo, const float* hi, float max_violation, float weight) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_chance_constraint(lo, hi, max_violation, weight);
    API_END
}

int bbmpc_get_constraint_violations(bbmpc_handle h, int32_t n_pop, float* prob_out, int32_t* first_step_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->constraint_violations(n_pop, prob_out, first_step_out);
    API_END
}

int bbmpc_evaluate_particles_dev(bbmpc_handle h, const float* d_state, const float* d_seq, int32_t n_pop, float* d_scores,
                                 float* d_returns) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_state);
    CHECK_PTR(d_seq);
    CHECK_PTR(d_scores);
    h->e->evaluate_particles_dev(d_state, d_seq, n_pop, d_scores, d_returns);
    API_END
}

int bbmpc_evaluate_particles(bbmpc_handle h, const float* state, const float* seq, int32_t n_pop, float* scores, float* returns) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(state);
    CHECK_PTR(seq);
    CHECK_PTR(scores);
    Engine& e = *h->e;
    if (!e.particles_on()) throw HipError(BBMPC_E_STATE, "particles are off: call bbmpc_set_particles first");
    if (n_pop < 1) throw HipError(BBMPC_E_INVALID, "n_pop must be >= 1");
    if (e.particle_user_reward() || e.constraint_on())
        e.require_particle_traj_fits((((long)n_pop + 63) / 64) * 64 * e.part_P);     // before the staging buffer
    const size_t nsc = (size_t)n_pop * e.A;
    HostStage st(e);
    const int q = st.in(seq, nsc * e.HU), sc = st.out(scores, nsc), ret = st.out(returns, nsc * e.part_P);
    st.upload();
    HIP_CHECK(hipMemcpyAsync(e.d_state.p, state, (size_t)e.A * e.S * 4, hipMemcpyHostToDevice, e.stream));   // (not a slot: DESIGN.md section 3a)
    e.evaluate_particles_dev(e.d_state.p, st[q], n_pop, st[sc], st[ret]);
    st.finish();
    API_END
}

}  // extern "C"
