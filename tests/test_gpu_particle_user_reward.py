"""HIP-source rewards under the particle evaluator on learned models: per-particle returns against
the NumPy helpers of tests/particle_util.py, ensemble_util.py and gaussian_util.py with a NumPy twin of each reward, the
built-in pendulum reward restated as a source against the built-in route, runtime parameters and the step index, the NaN
rule, clipped actions under PI2, all six optimizers, CVaR, trajectory distributions, the lifecycle and the Python classes.
Every comparison runs on injected process noise."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import ensemble_util as EU
from tests import gaussian_util as GU
from tests import particle_user_reward_util as RU
from tests import particle_util as PU
from tests import risk_util as RK
from tests import traj_particles_util as TP
from tests.test_ensemble_cpu import member_evaluators, network
from tests.test_gaussian_cpu import member_heads

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device visible"
    return _lib


def _handle(L, spec, params, stats, A, H, reward=None, opt=None, N=0, iters=0, k=0, lo=None, hi=None, **kw):
    """A BBMPC_DYN_MLP handle with member 0 installed; reward: a built-in kind, or None for BBMPC_REW_USER."""
    from blackbox_mpc_amd.engine import Engine
    from tests.test_gpu_activations import CODE
    dims, acts, S, U, _ = spec
    eng = Engine(opt if opt is not None else L.OPT_NONE, L.DYN_MLP, L.REW_USER if reward is None else reward,
                 lo or [-1.0] * U, hi or [1.0] * U, dim_s=S, num_agents=A, planning_horizon=H, population_size=N,
                 max_iterations=iters, num_elite=k, **kw)
    eng.set_mlp(params[0][0], params[0][1], [CODE[a] for a in acts], stats)
    return eng


def _pend(L, A, H, src=RU.MIXED_REWARD, reward_np=RU.mixed_np, num_params=0, E=1, **kw):
    """PEND_MLP with a user reward: (handle, members' parameters, oracle evaluators carrying the NumPy twin)."""
    spec = network("PEND_MLP")
    params, stats, evs = member_evaluators(spec, E)
    eng = _handle(L, spec, params, stats, A, H, **kw)
    if src is not None:
        eng.set_reward_source(src, num_params)
    return eng, params, [O.Evaluator(reward_np, ev.handler) for ev in evs]


def _inputs(A, N, H, P, seed, S=3, U=1):
    rng = np.random.default_rng(seed)
    states = (O.pendulum_start_states(A) if S == 3 else O.cheetah_start_states(A, S)).astype(F)
    return states, rng.uniform(-1, 1, (N, A, H, U)).astype(F), rng.standard_normal((A, P, H, S)).astype(F)


SIGMA3 = np.full(3, 0.02, F)


# ---- 1. returns against the NumPy helper ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,A,P,H", [("PEND_MLP", 13, 2, 4, 5), ("NARROW", 5, 2, 4, 3)])
def test_returns_match_the_helper(L, name, N, A, P, H):
    spec = network(name)
    S, U = spec[2], spec[3]
    params, stats, evs = member_evaluators(spec, 1)
    eng = _handle(L, spec, params, stats, A, H)
    eng.set_reward_source(RU.MIXED_REWARD)
    states, seq, eps = _inputs(A, N, H, P, 4100, S, U)
    sigma = np.full(S, 0.02, F)
    eng.set_particles(P, sigma, 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    eng.set_profiling(True)
    scores, got = eng.evaluate_particles(states, seq)
    assert eng.get_profile()[2] == "k_rollout_mlp_particles"
    want = PU.particle_returns(O.Evaluator(RU.mixed_np, evs[0].handler), states, seq, eps, sigma, P)
    assert got.shape == (N, P, A) and np.all(np.isfinite(want))
    print("[particle user reward %s] max |dev - helper| = %.3e" % (name, np.abs(got.astype(np.float64) - want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)
    np.testing.assert_allclose(scores, PU.aggregate64(got, 0.0), rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(eng.evaluate(states, seq), scores)


# ---- 2. same arithmetic, other route ----------------------------------------------------------------------------------
def test_restated_pendulum_reward_agrees_with_the_builtin_route(L):
    """Observed on an MI355X: see profiles/particle_user_reward.md."""
    N, A, P, H = 13, 2, 4, 5
    spec = network("PEND_MLP")
    params, stats, _ = member_evaluators(spec, 1)
    user = _handle(L, spec, params, stats, A, H)
    user.set_reward_source(RU.PENDULUM_AS_EXECUTED)
    builtin = _handle(L, spec, params, stats, A, H, reward=L.REW_PENDULUM)
    states, seq, eps = _inputs(A, N, H, P, 4200)
    out = []
    for eng in (user, builtin):
        eng.set_particles(P, SIGMA3, 0.0)
        eng.inject_noise(L.NOISE_PROCESS, eps)
        out.append(eng.evaluate_particles(states, seq)[1])
    diff = np.abs(out[0].astype(np.float64) - out[1])
    print("[particle user reward, restated pendulum] max |user - builtin| = %.3e (max |return| %.3e), identical bits: %s"
          % (diff.max(), np.abs(out[1]).max(), np.array_equal(out[0], out[1])))
    np.testing.assert_allclose(out[0], out[1], rtol=1e-3, atol=0)


# ---- 3. members and heads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,heads", [(2, False), (1, True), (2, True)])
def test_members_and_heads(L, E, heads):
    N, A, P, H = 9, 2, 4, 4
    eng, params, evs = _pend(L, A, H, E=E)
    states, seq, eps = _inputs(A, N, H, P, 4300 + 10 * E + heads)
    eng.set_particles(P, SIGMA3, 0.0)
    if E > 1:
        eng.set_mlp_ensemble(params)
    if heads:
        raw, bounds, hs = member_heads(network("PEND_MLP"), evs)
        eng.set_mlp_logvar_head(raw, *bounds)
        want = GU.gaussian_particle_returns(evs, hs, states, seq, eps, SIGMA3, P)
    else:
        want = EU.ensemble_particle_returns(evs, states, seq, eps, SIGMA3, P)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    eng.set_profiling(True)
    _, got = eng.evaluate_particles(states, seq)
    assert eng.get_profile()[2] == ("k_rollout_mlp_particles_gauss" if heads else "k_rollout_mlp_particles_ens")
    print("[particle user reward E=%d heads=%s] max |dev - helper| = %.3e" % (E, heads, np.abs(got.astype(np.float64) - want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)
    if E > 1:                                            # the members differ, so a wrong slot shows
        assert np.any(got[:, 0] != got[:, 1])


# ---- 4. parameters and the step index ---------------------------------------------------------------------------------
def test_per_agent_parameters_and_the_step_index(L):
    N, A, P, H = 13, 2, 4, 5
    eng, _, evs = _pend(L, A, H, src=RU.GOAL_STEP_REWARD, num_params=2)
    states, seq, eps = _inputs(A, N, H, P, 4400)
    eng.set_particles(P, SIGMA3, 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    with pytest.raises(L.BBMPCError) as ei:              # declared, not yet set
        eng.evaluate_particles(states, seq)
    assert ei.value.code == L.E_STATE
    compiles = eng.compile_count()
    results = []
    for goals in ([[0.8, 0.1], [-0.4, 0.7]], [[-0.2, 0.3], [0.6, 0.05]]):
        eng.set_user_params(L.USER_KIND_REWARD, np.array(goals, F))
        _, got = eng.evaluate_particles(states, seq)
        want = PU.particle_returns(O.Evaluator(RU.GoalStepReward(goals), evs[0].handler), states, seq, eps, SIGMA3, P)
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)
        results.append(got)
    assert np.abs(results[0] - results[1]).max() > 10 * 1e-3 * H    # the returns moved with the parameters, far beyond the tolerance
    assert eng.compile_count() == compiles


# ---- 5. the NaN rule, per particle ------------------------------------------------------------------------------------
def test_nan_rule_per_particle(L):
    N, A, P, H = 13, 2, 4, 5
    eng, _, _ = _pend(L, A, H, src=RU.NAN_ABOVE_REWARD)
    states, seq, eps = _inputs(A, N, H, P, 4500)
    sigma = np.array([0.02, 0.02, 1.0], F)
    eng.set_particles(P, sigma, 1.5)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    s0, r0 = eng.evaluate_particles(states, seq)
    assert np.all(np.isfinite(r0)) and np.all(r0 > F(-1e5))
    hot = eps.copy()
    hot[1, 2, 3, 2] = 200.0                              # particle 2 of agent 1 crosses the threshold at step 3, nobody else
    eng.inject_noise(L.NOISE_PROCESS, hot)
    s1, r1 = eng.evaluate_particles(states, seq)
    assert np.all(r1[:, 2, 1] == F(-1e6))
    keep = np.arange(P) != 2
    np.testing.assert_array_equal(r1[:, keep, :], r0[:, keep, :])
    np.testing.assert_array_equal(r1[:, :, 0], r0[:, :, 0])
    assert np.all(np.isfinite(s1))
    np.testing.assert_allclose(s1, PU.aggregate64(r1, 1.5), rtol=1e-5)


# ---- 6. clipped actions -----------------------------------------------------------------------------------------------
def test_pi2_lockstep_scores_the_clipped_actions(L):
    N, A, H, iters, P = 64, 2, 6, 2, 4
    lo, hi = [-0.5], [0.5]
    eng, _, evs = _pend(L, A, H, opt=L.OPT_PI2, N=N, iters=iters, lo=lo, hi=hi)
    rng = np.random.default_rng(4600)
    eps = rng.standard_normal((iters, A, P, H, 3)).astype(F)
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]}
    start = np.full((A, H, 1), 0.4, F)                   # a mean next to the upper bound: sigma = 0.25, so draws leave the box
    eng.set_trace(True)
    eng.set_particles(P, SIGMA3, 0.5)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    eng.inject_noise(L.NOISE_PROCESS, eps)
    eng.set_state("prev_mean", start)
    states = O.pendulum_start_states(A)
    act, _, _ = eng.optimize(states)
    hip_r = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(iters)]

    def lock(it, r_o):
        print("[particle user reward pi2 it %d] max |dev - oracle| = %.3e" % (it, np.abs(hip_r[it].astype(np.float64) - r_o).max()))
        np.testing.assert_allclose(hip_r[it], r_o, rtol=1e-3, atol=1e-3 * H)
        return hip_r[it]
    helper = PU.ParticleEvaluator(RU.mixed_np, evs[0].handler, P, SIGMA3, 0.5, eps)
    pi2 = O.PI2(helper, lo, hi, horizon=H, max_iterations=iters, population=N, num_agents=A)
    pi2.prev = start.copy()
    act_o = pi2._optimize(states, noise, rewards_override=lock)
    raw0 = ((noise["trunc"][0] * F(0.25)).astype(F) + start[None]).astype(F)
    assert (raw0 > F(0.5)).mean() > 0.1 and pi2.trace[0]["penalty"].max() > 0          # not vacuous: many draws were clipped
    # the reward reads the action: scoring the unclipped draws moves the returns by far more than the tolerance
    unclipped = PU.particle_returns(helper, states, raw0, eps[0], SIGMA3, P)
    clipped = PU.particle_returns(helper, states, np.clip(raw0, F(-0.5), F(0.5)), eps[0], SIGMA3, P)
    assert np.abs(unclipped - clipped).max() > 10 * 1e-3 * H
    for it in range(iters):
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_SAMPLES), pi2.trace[it]["samples"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), pi2.trace[it]["mean"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(act, act_o, rtol=0, atol=2e-5)


# ---- 7. all six optimizers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["RANDOM_SEARCH", "CEM", "PI2", "PSO", "SPSA", "CMAES"])
def test_every_optimizer_scores_through_the_particles(L, opt_name):
    """tests/test_gpu_particles.py::test_other_optimizers_score_through_the_particles on the user-reward handle: the step
    completes, iteration 0's traced rewards are what evaluate_particles gives for its candidates minus their bound penalty,
    the action is finite and inside the bounds."""
    N, A, H, P = 32, 1, 6, 4
    rng = np.random.default_rng(4700)
    eps = rng.standard_normal((1, A, P, H, 3)).astype(F)
    eng, _, _ = _pend(L, A, H, opt=getattr(L, "OPT_" + opt_name), N=N, iters=1, k=8)
    eng.set_trace(True)
    eng.set_particles(P, SIGMA3, 1.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    pen = np.zeros((N, A), F)
    cands = None
    if opt_name == "PSO":                                 # the constructor's swarm: every position zero
        cands = [np.zeros((N, A, H, 1), F)]
    elif opt_name == "SPSA":                              # mean (the bounds' midpoint, 0) +- c_0 * delta, c_0 = 0.3
        delta = np.where(rng.random((N, A, H, 1)) < 0.5, F(-1), F(1)).astype(F)
        eng.inject_noise(L.NOISE_RADEMACHER, delta[None])
        cands = [(F(0.3) * delta).astype(F), (F(-0.3) * delta).astype(F)]
    elif opt_name == "CMAES":                             # m + sigma * B D z with m = 0, sigma = (hi - lo) / 4 = 0.5, B = D = I
        z = rng.standard_normal((N, A, H, 1)).astype(F)
        eng.inject_noise(L.NOISE_NORMAL, z[None])
        x = (F(0.5) * z).astype(F)
        feas = np.clip(x, F(-1), F(1))
        d = (x - feas).reshape(N, A, -1)
        nrm = O.sqrt32(O.seq_sum((d * d).astype(F), axis=2))
        pen = (nrm * nrm).astype(F)
        assert pen.max() > 0
        cands = [feas]
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    assert np.all(np.isfinite(act)) and np.all(act >= -1.0) and np.all(act <= 1.0) and np.all(np.isfinite(nxt)) and np.all(np.isfinite(rew))
    traced = eng.get_trace(0, L.TRACE_REWARDS)
    if cands is None:                                     # RandomSearch / CEM / PI2 at the constructor distribution: no draw leaves the box
        cands = [eng.get_trace(0, L.TRACE_SAMPLES)]
    want = np.concatenate([(eng.evaluate_particles(states, c)[0] - pen).astype(F) for c in cands])
    np.testing.assert_allclose(traced, want, rtol=1e-6, atol=1e-5)
    # the record is the noise-free one-step prediction with the user's reward
    np.testing.assert_allclose(rew, RU.mixed_np(states, act, nxt), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("form", ["elite_carry", "colored_noise"])
def test_cem_with_carried_elites_and_colored_noise(L, form):
    N, A, H, P = 32, 2, 6, 4
    eng, _, _ = _pend(L, A, H, opt=L.OPT_CEM, N=N, iters=2, k=8)
    eng.set_particles(P, SIGMA3, 0.5)
    if form == "elite_carry":
        eng.set_elite_carry(2, 2)
    else:
        from blackbox_mpc_amd.utils.colored_noise import colored_noise_mixing
        eng.set_sampling_correlation(colored_noise_mixing(H, 1.0))
    s = O.pendulum_start_states(A)
    for _ in range(2):
        act, nxt, _ = eng.optimize(s)
        assert np.all(np.isfinite(act)) and np.all(act >= -1.0) and np.all(act <= 1.0) and np.all(np.isfinite(nxt))
        s = nxt


# ---- 8. CVaR ----------------------------------------------------------------------------------------------------------
def test_cvar_is_the_mean_of_the_worst_returns(L):
    N, A, P, H = 13, 2, 8, 5
    eng, _, _ = _pend(L, A, H)
    states, seq, eps = _inputs(A, N, H, P, 4800)
    eng.set_particles(P, SIGMA3, 0.0)
    eng.set_particle_risk(L.RISK_CVAR, 2)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    scores, returns = eng.evaluate_particles(states, seq)
    np.testing.assert_array_equal(scores, RK.cvar32(returns, 2))
    np.testing.assert_allclose(scores, RK.cvar64(returns, 2), rtol=1e-6)


# ---- 9. trajectory distributions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_agent", [False, True])
def test_trajectory_distribution(L, per_agent):
    A, P, Hq = 2, 4, 7
    B = 2 * A if per_agent else 5
    goals = np.array([[0.8, 0.1], [-0.4, 0.7]], F)
    if per_agent:
        eng, _, _ = _pend(L, A, 3, src=RU.GOAL_STEP_REWARD, num_params=2)
        eng.set_user_params(L.USER_KIND_REWARD, goals)
    else:
        eng, _, _ = _pend(L, A, 3)
    rng = np.random.default_rng(4900)
    th = rng.uniform(-np.pi, np.pi, B)
    states = np.stack([np.cos(th), np.sin(th), rng.uniform(-1, 1, B)], axis=1).astype(F)
    seq = rng.uniform(-1, 1, (B, Hq, 1)).astype(F)
    eps = rng.standard_normal((B, P, Hq, 3)).astype(F)
    eng.set_particles(P, SIGMA3, 0.0)
    ranks = [0, P - 1]
    smean, sstd, rmean, rstd, squant, rquant, ps, pr = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True,
                                                                                         quantile_ranks=ranks)
    m2 = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)
    np.testing.assert_array_equal(m2[5], pr)
    np.testing.assert_array_equal(m2[2], rmean)
    assert pr.shape == (B, P, Hq) and np.all(np.isfinite(pr)) and np.any(pr != 0)
    # the reward of the returned particle states: the current state is the row's start state at t = 0, then the state before
    cur = np.concatenate([np.broadcast_to(states[:, None, None], (B, P, 1, 3)), ps[:, :, :-1]], axis=2)
    act = np.broadcast_to(seq[:, None], (B, P, Hq, 1))
    want = np.empty((B, P, Hq), F)
    for t in range(Hq):
        c, a, n = (x[:, :, t].reshape(B * P, -1) for x in (cur, act, ps))
        if per_agent:
            rows = np.repeat(goals[np.arange(B) // (B // A)], P, axis=0)
            want[:, :, t] = RU.goal_step_np(c, a, n, rows, t).reshape(B, P)
        else:
            want[:, :, t] = RU.mixed_np(c, a, n).reshape(B, P)
    # same inputs, a handful of float32 operations of O(1) values on both sides
    np.testing.assert_allclose(pr, want, rtol=1e-5, atol=1e-6)
    TP.check_moments(rmean, rstd, pr, "particle user reward, rewards")
    TP.check_moments(smean, sstd, ps, "particle user reward, states")
    np.testing.assert_array_equal(rquant, RK.nearest_rank(pr, ranks, 1))
    np.testing.assert_array_equal(squant, RK.nearest_rank(ps, ranks, 1))


# ---- 10. lifecycle and refusals ---------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(L):
    from blackbox_mpc_amd.engine import Engine
    N, A, P, H = 13, 2, 4, 5
    eng, params, _ = _pend(L, A, H)
    states, seq, eps = _inputs(A, N, H, P, 5000)
    before = eng.evaluate(states, seq)
    eng.set_particles(P, SIGMA3, 0.0)
    assert not np.array_equal(eng.evaluate(states, seq), before)
    eng.set_particles(0)
    np.testing.assert_array_equal(eng.evaluate(states, seq), before)

    # no source yet
    spec = network("PEND_MLP")
    bare, _, _ = _pend(L, A, H, src=None)
    bare.set_particles(P, SIGMA3, 0.0)
    for call in (lambda: bare.evaluate_particles(states, seq),
                 lambda: bare.predict_trajectory_particles(states, seq[0], eps=None)):
        with pytest.raises(L.BBMPCError) as ei:
            call()
        assert ei.value.code == L.E_STATE and "bbmpc_set_reward_source" in str(ei.value)
    bare.set_reward_source(RU.MIXED_REWARD)
    assert np.all(np.isfinite(bare.evaluate_particles(states, seq)[1]))

    # a torch callable: refused when it computes, and the handle stays usable
    import torch
    cb, _, _ = _pend(L, A, H, src=None)
    from blackbox_mpc_amd.utils.device_functions import TorchRewardFunction
    plug = TorchRewardFunction(lambda c, a, n: -(n[:, 0] * n[:, 0]))
    cb.set_reward_callback(plug.make_callback(3, 1, cb.device))
    det = cb.evaluate(states, seq)
    cb.set_particles(P, SIGMA3, 0.0)
    with pytest.raises(L.BBMPCError) as ei:
        cb.evaluate_particles(states, seq)
    assert ei.value.code == L.E_UNSUPPORTED and "HIP-source reward" in str(ei.value)
    cb.set_particles(0)
    np.testing.assert_array_equal(cb.evaluate(states, seq), det)
    assert torch.cuda.is_available()

    # 22 * 2 * 3 * (2^22 * 4) = 2^31 + ... trajectory elements: refused before anything is allocated (the arrays are never touched)
    big, _, _ = _pend(L, 2, 22)
    big.set_particles(4, SIGMA3, 0.0)
    n_big = 1 << 22
    with pytest.raises(L.BBMPCError) as ei:
        big.evaluate_particles(O.pendulum_start_states(2), np.zeros((n_big, 2, 22, 1), F))
    assert ei.value.code == L.E_UNSUPPORTED and "2^31" in str(ei.value)
    assert np.all(np.isfinite(big.evaluate_particles(O.pendulum_start_states(2), np.zeros((3, 2, 22, 1), F))[1]))

    # what stays refused
    user = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_USER, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=5)
    user.set_reward_source(RU.MIXED_REWARD)
    dyn = Engine(L.OPT_NONE, L.DYN_USER, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=5)
    for handle, word in ((user, "reward"), (dyn, "dynamics")):
        with pytest.raises(L.BBMPCError) as ei:
            handle.set_particles(2, SIGMA3)
        assert ei.value.code == L.E_UNSUPPORTED and word in str(ei.value)
    xf, _, _ = _pend(L, 1, 5)
    xf.set_inverse_transform_source("""
__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {
    for (int i = 0; i < S; ++i) next[i] = cur[i] + dev[i];
}
""")
    with pytest.raises(L.BBMPCError) as ei:
        xf.set_particles(2, SIGMA3)
    assert ei.value.code == L.E_UNSUPPORTED and "transform" in str(ei.value)


# ---- 11. Python -------------------------------------------------------------------------------------------------------
def test_policy_with_a_hip_reward_and_particles(L):
    from blackbox_mpc_amd.dynamics_functions import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.trajectory_evaluators import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.device_functions import HipRewardFunction
    act_space, obs_space = Box([-1.0], [1.0]), Box([-1, -1, -8], [1, 1, 8])
    H, P = 6, 4
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=DeterministicMLP([4, 16, 16, 3], ["tanh", "tanh", None], seed=3),
                                    true_model=False, is_normalized=False)
    reward = HipRewardFunction(RU.GOAL_STEP_REWARD, num_params=2)
    reward.set_params(np.array([0.8, 0.1], F))
    ev = ParticleTrajectoryEvaluator(reward, handler, P, 0.02, risk_alpha=0.5)
    pol = MPCPolicy(trajectory_evaluator=ev, env_action_space=act_space, env_observation_space=obs_space, optimizer_name="CEM",
                    num_agents=1, planning_horizon=H, population_size=32, max_iterations=2, num_elite=8, seed=5)
    pol.keep_plan(True)
    obs = np.array([1.0, 0.0, 0.0], F)
    for t in range(3):
        a, n, r = pol.act(obs, t)
        assert a.shape == (1,) and np.all(np.isfinite(a)) and np.all(np.abs(a) <= 1.0) and np.all(np.isfinite(n)) and np.isfinite(r)
    out = pol.plan_distribution(obs[None], quantiles=[0.05, 0.95])
    actions, smean, sstd, rmean, rstd, squant, rquant = out
    assert actions.shape == (1, H, 1) and smean.shape == sstd.shape == (1, H, 3) and rmean.shape == rstd.shape == (1, H)
    assert squant.shape == (1, 2, H, 3) and rquant.shape == (1, 2, H) and np.all(np.isfinite(rmean)) and np.any(rmean != 0)
    # set_params between two computations: uploaded before the particles run, never recompiled
    seq = np.random.default_rng(5100).uniform(-1, 1, (9, 1, H, 1)).astype(F)
    r0 = ev.particle_returns(obs[None], seq)
    eng = ev._engine(1, H)
    compiles = eng.compile_count()
    reward.set_params(np.array([-0.5, 0.6], F))
    r1 = ev.particle_returns(obs[None], seq)
    assert r0.shape == (9, P, 1) and np.abs(r1 - r0).max() > 1e-2
    assert ev._engine(1, H).compile_count() == compiles
    scores = ev(obs[None], seq)
    np.testing.assert_array_equal(scores, RK.cvar32(r1, 2))
    d = ev.predict_trajectory_distribution(obs[None], seq[0], return_particles=True)
    assert d[5].shape == (1, P, H) and np.any(d[5] != 0)
