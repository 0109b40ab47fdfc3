"""CVaR scoring and quantile bands of the particle evaluator on the GPU (include/bbmpc.h: bbmpc_set_particle_risk,
bbmpc_predict_trajectory_quantiles) against the NumPy statements of tests/risk_util.py: the selection is exact given the
returns / particle tensors the same call gave back, so most comparisons are bit for bit.

Shapes: N = 37 candidates (no multiple of the four waves of a workgroup, nor of 64) on A = 2 agents, P in {1, 5, 64} (one
lane, a partial wave, a full wave); the quantile kernel on B = 3, Hq = 5 (45 + 15 waves: a partial last workgroup)."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import particle_util as PU
from tests import risk_util as RU
from tests.test_particles_cpu import AGG_SIGMA, R_ATOL, R_RTOL, pendulum_case

pytestmark = pytest.mark.gpu

F = np.float32
LO, HI = [-2.0], [2.0]
TINY = ([4, 8, 3], ["tanh", None], 3, 1, "pendulum")


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device visible"
    return _lib


def _engine(L, opt, A, H, N=0, iters=0, k=0, **kw):
    from blackbox_mpc_amd.engine import Engine
    return Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, LO, HI, dim_s=3, num_agents=A, planning_horizon=H,
                  population_size=N, max_iterations=iters, num_elite=k, **kw)


def _tiny_mlp(L, A, H, members=2):
    from tests.test_gpu_mlp import _problem
    dims, acts, S, U, reward = TINY
    eng, ev, lo, hi = _problem(L, dims, acts, S, U, reward, True, A=A, H=H)
    if members > 1:
        eng.set_mlp_ensemble([O.make_mlp_params(dims, seed=42 + 7 * e) for e in range(members)])
    return eng


class CvarEvaluator(PU.ParticleEvaluator):
    """particle_util.ParticleEvaluator scoring with cvar32 of its float32 returns"""

    def __init__(self, reward, handler, num_particles, sigma, k, eps):
        super().__init__(reward, handler, num_particles, sigma, 0.0, eps)
        self.k = k

    def __call__(self, current_states, action_sequences, return_final_state=False):
        super().__call__(current_states, action_sequences, return_final_state)
        return RU.cvar32(self.last_returns, self.k)


# ---- 1. the score ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5, 64])
def test_pendulum_scores_are_cvar_of_the_returned_returns(L, P):
    N, A, H = 37, 2, 4
    states, seq, eps = pendulum_case(N, A, P, H)
    eng = _engine(L, L.OPT_NONE, A, H)
    eng.set_particles(P, AGG_SIGMA, 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    mean_scores, mean_returns = eng.evaluate_particles(states, seq)
    for k in sorted({1, 2, P}):
        if k > P:
            continue
        eng.set_particle_risk(L.RISK_CVAR, k)
        scores, returns = eng.evaluate_particles(states, seq)
        np.testing.assert_array_equal(returns, mean_returns)                   # the rollouts do not depend on the rule
        np.testing.assert_array_equal(scores, RU.cvar32(returns, k))
        np.testing.assert_array_equal(eng.evaluate(states, seq), scores)
        err = np.abs(scores.astype(np.float64) - RU.cvar64(returns, k))
        bound = 64.0 * P * 2.0 ** -24 * np.abs(returns.astype(np.float64)).max(axis=1)
        print("[cvar pendulum P=%d k=%d] max err / bound = %.3e" % (P, k, (err / bound).max()))
        assert np.all(err <= bound)
        if k == 1:
            np.testing.assert_array_equal(scores, returns.min(axis=1))
        if k == P:                                                             # device against device: the kappa = 0 mean's bits
            np.testing.assert_array_equal(scores, mean_scores)
    if P > 1:
        assert np.any(RU.cvar32(mean_returns, 1) != mean_scores)
    eng.set_particle_risk(L.RISK_MEAN_STD, 0)
    np.testing.assert_array_equal(eng.evaluate_particles(states, seq)[0], mean_scores)


def test_equal_particles_score_their_return_for_every_k(L):
    N, A, P, H = 37, 2, 4, 4
    states, seq, eps = pendulum_case(N, A, P, H)
    eng = _engine(L, L.OPT_NONE, A, H)
    eng.set_particles(P, np.zeros(3, F), 0.0)                  # sigma = 0 on one model: all particles equal
    eng.inject_noise(L.NOISE_PROCESS, eps)
    for k in (1, 2, 3, 4):
        eng.set_particle_risk(L.RISK_CVAR, k)
        scores, returns = eng.evaluate_particles(states, seq)
        assert np.all(returns == returns[:, :1])
        # (the float32 sum of k equal values over k: exact for k = 1, 2, 4; for k = 3 it is what cvar32 states)
        np.testing.assert_array_equal(scores, RU.cvar32(returns, k))
        if k != 3:
            np.testing.assert_array_equal(scores, returns[:, 0])
        else:
            np.testing.assert_allclose(scores, returns[:, 0], rtol=2 ** -22, atol=0)


def test_learned_ensemble_worst_case_is_the_row_minimum(L):
    N, A, P, H = 19, 1, 4, 3
    eng = _tiny_mlp(L, A, H, members=2)
    rng = np.random.default_rng(19)
    states = O.pendulum_start_states(A).astype(F)
    seq = rng.uniform(-1, 1, (N, A, H, 1)).astype(F)
    eng.set_particles(P, np.full(3, 0.02, F), 0.0)
    eng.set_particle_risk(L.RISK_CVAR, 1)
    eng.inject_noise(L.NOISE_PROCESS, rng.standard_normal((A, P, H, 3)).astype(F))
    scores, returns = eng.evaluate_particles(states, seq)
    np.testing.assert_array_equal(scores, returns.min(axis=1))
    assert np.all(np.ptp(returns, axis=1) > 0)


# ---- 2. the penalty path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["PI2", "CMAES"])
def test_penalty_and_write_back_under_cvar(L, opt_name):
    """One control step with trace and injected draws, as tests/test_gpu_particles.py drives it: the traced rewards of
    iteration 0 are cvar32 of the returns of the clipped candidates minus the bound penalty (that file's tolerance), and the
    traced samples are the clipped candidates."""
    N, A, H, P, k = 37, 1, 6, 5, 2
    rng = np.random.default_rng(31)
    eps = rng.standard_normal((1, A, P, H, 3)).astype(F)
    eng = _engine(L, L.OPT_PI2 if opt_name == "PI2" else L.OPT_CMAES, A, H, N=N, iters=1, k=8)
    eng.set_trace(True)
    eng.set_particle_risk(L.RISK_CVAR, k)                       # before set_particles: the order is free
    eng.set_particles(P, AGG_SIGMA, 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    helper = O.PI2(None, LO, HI, horizon=H, max_iterations=1, population=N, num_agents=A)
    if opt_name == "PI2":                                       # mean 1, unit variance, draws in [-2, 2]: samples up to 3
        xi = O.truncated_normal_noise(rng, (N, A, H, 1))
        eng.inject_noise(L.NOISE_TRUNC_NORMAL, xi[None])
        mean = np.full((A, H, 1), 1.0, F)
        eng.set_state("prev_mean", mean)
        raw = ((xi * O.sqrt32(helper.var)).astype(F) + mean).astype(F)
    else:                                                       # m + sigma * B D z with m = 0, sigma = 1, B = D = I: the draws
        raw = rng.standard_normal((N, A, H, 1)).astype(F)
        eng.inject_noise(L.NOISE_NORMAL, raw[None])
    feas = helper._clip_h(raw)
    pen = helper._penalty(raw, feas)
    assert (pen > 0).sum() >= 3 and (pen == 0).sum() >= 3
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    assert np.all(np.isfinite(act)) and np.all(act >= -2.0) and np.all(act <= 2.0)
    samples = eng.get_trace(0, L.TRACE_SAMPLES)
    np.testing.assert_allclose(samples, feas, rtol=0, atol=2e-5)
    assert np.all(samples >= -2.0) and np.all(samples <= 2.0)
    scores, returns = eng.evaluate_particles(states, samples)
    np.testing.assert_array_equal(scores, RU.cvar32(returns, k))
    np.testing.assert_allclose(eng.get_trace(0, L.TRACE_REWARDS), (RU.cvar32(returns, k) - pen).astype(F), rtol=1e-6, atol=1e-5)


# ---- 3. the optimizers ----------------------------------------------------------------------------------------------
def _policy(name, risk_alpha, P=5, seed=3, **kw):
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.trajectory_evaluators import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    act_space, obs_space = Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8])
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=PendulumTrueModel(), true_model=True)

    def evaluator(alpha):
        return ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=P, process_noise_std=AGG_SIGMA, risk_alpha=alpha)
    settings = dict(population_size=48, max_iterations=2)
    if name in ("CEM", "CMA-ES"):
        settings["num_elite"] = 8
    if name == "RandomSearch":
        settings.pop("max_iterations")
    pol = MPCPolicy(trajectory_evaluator=evaluator(risk_alpha), env_action_space=act_space, env_observation_space=obs_space,
                    optimizer_name=name, num_agents=2, planning_horizon=5, seed=seed, **settings, **kw)
    return pol, evaluator


@pytest.mark.parametrize("name", ["CEM", "PI2", "PSO", "RandomSearch", "SPSA", "CMA-ES"])
def test_every_optimizer_plans_on_the_cvar_score(L, name):
    pol, _ = _policy(name, 0.4)
    eng = pol._optimizer._engine
    assert eng.risk == (L.RISK_CVAR, 2) and eng.P == 5
    obs = O.pendulum_start_states(2)
    action, nxt, rew = pol.act(obs, 0)
    assert action.shape == (2, 1) and np.all(np.isfinite(action)) and np.all(action >= -2.0) and np.all(action <= 2.0)
    assert np.all(np.isfinite(nxt)) and np.all(np.isfinite(rew))
    # equal calls on equal policies give equal bits, and the rule is the evaluator's
    again, _ = _policy(name, 0.4)
    np.testing.assert_array_equal(again.act(obs, 0)[0], action)
    other, _ = _policy(name, None)
    assert other._optimizer._engine.risk == (L.RISK_MEAN_STD, 0)


def test_cem_lockstep_with_the_numpy_replay(L):
    N, A, H, iters, ne, P, k = 64, 1, 5, 2, 8, 4, 2
    rng = np.random.default_rng(17)
    eps = rng.standard_normal((iters, A, P, H, 3)).astype(F)
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]}
    eng = _engine(L, L.OPT_CEM, A, H, N=N, iters=iters, k=ne)
    eng.set_trace(True)
    eng.set_particles(P, AGG_SIGMA, 0.5)                        # (kappa is ignored under CVaR)
    eng.set_particle_risk(L.RISK_CVAR, k)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    eng.inject_noise(L.NOISE_PROCESS, eps)
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    hip_el = [eng.get_trace(it, L.TRACE_ELITES) for it in range(iters)]
    hip_r = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(iters)]
    # iteration 0 on the device's own returns of the traced samples: the selection is exact given those
    s0, r0 = eng.evaluate_particles(states, eng.get_trace(0, L.TRACE_SAMPLES))
    np.testing.assert_array_equal(s0, RU.cvar32(r0, k))
    np.testing.assert_allclose(hip_r[0], RU.cvar32(r0, k), rtol=1e-6, atol=1e-5)

    def select(it, r_o, own):                                   # the forced-elites hook of tests/test_gpu_particles.py
        np.testing.assert_allclose(hip_r[it], r_o, rtol=R_RTOL, atol=R_ATOL)
        for a in range(A):
            he = hip_el[it][a]
            if set(own[a]) != set(he):
                kth = np.sort(r_o[:, a])[::-1][ne - 1]
                for n in set(own[a]) ^ set(he):
                    assert abs(r_o[n, a] - kth) <= R_ATOL + R_RTOL * abs(kth)
            np.testing.assert_array_equal(he, O.topk_desc(hip_r[it][:, a], ne))
        return hip_el[it]
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
    cem = O.CEM(CvarEvaluator(ev.reward, ev.handler, P, AGG_SIGMA, k, eps), LO, HI, horizon=H, max_iterations=iters, population=N,
                num_elite=ne, num_agents=A)
    cem._optimize(states, noise, forced_elites=select)
    for it in range(iters):
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_SAMPLES), cem.trace[it]["samples"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), cem.trace[it]["mean"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(act, cem.trace[-1]["mean"][:, 0], rtol=0, atol=2e-5)


def test_scores_follow_the_evaluator(L):
    """The staleness rule: the engine an evaluator works on is reset by whichever evaluator uses it next."""
    pol, evaluator = _policy("CEM", 0.4)
    cvar_ev, mean_ev = pol._optimizer._trajectory_evaluator, evaluator(None)
    obs = O.pendulum_start_states(2)
    a_cvar = pol.act(obs, 0)[0]
    pol._optimizer.set_trajectory_evaluator(mean_ev)
    assert pol._optimizer._engine.risk == (L.RISK_MEAN_STD, 0)
    pol._optimizer.set_trajectory_evaluator(cvar_ev)
    assert pol._optimizer._engine.risk == (L.RISK_CVAR, 2)
    np.testing.assert_array_equal(pol.act(obs, 0)[0], a_cvar)   # (a fresh engine with the same seed)
    # the evaluators' own calls share nothing but the rule they carry; one engine handed from one to the other follows
    seq = np.random.default_rng(5).uniform(-2, 2, (9, 2, 5, 1)).astype(F)
    r = cvar_ev.particle_returns(obs, seq)
    np.testing.assert_array_equal(cvar_ev(obs, seq), RU.cvar32(r, 2))
    eng = cvar_ev._particle_engine(seq)
    assert eng.risk == (L.RISK_CVAR, 2)
    mean_ev._apply_particles(eng)
    assert eng.risk == (L.RISK_MEAN_STD, 0)
    np.testing.assert_array_equal(eng.evaluate(obs, seq), PU.aggregate32(eng.evaluate_particles(obs, seq)[1], 0.0))
    cvar_ev._apply_particles(eng)
    np.testing.assert_array_equal(eng.evaluate(obs, seq), cvar_ev(obs, seq))
    # fewer particles than the tail another evaluator left behind
    small = type(cvar_ev)(cvar_ev._reward_function, cvar_ev._system_dynamics_handler, num_particles=1, process_noise_std=AGG_SIGMA)
    small._apply_particles(eng)
    assert eng.P == 1 and eng.risk == (L.RISK_MEAN_STD, 0)


# ---- 4. quantiles ---------------------------------------------------------------------------------------------------
def _check_quantiles(out, ranks, P):
    sm, ss, rm, rs, sq, rq, ps, pr = out
    np.testing.assert_array_equal(sq, RU.nearest_rank(ps, ranks, 1))
    np.testing.assert_array_equal(rq, RU.nearest_rank(pr, ranks, 1))
    for l, r in enumerate(ranks):
        if r == 0:
            np.testing.assert_array_equal(sq[:, l], ps.min(axis=1))
            np.testing.assert_array_equal(rq[:, l], pr.min(axis=1))
        if r == P - 1:
            np.testing.assert_array_equal(sq[:, l], ps.max(axis=1))
            np.testing.assert_array_equal(rq[:, l], pr.max(axis=1))


@pytest.mark.parametrize("P", [1, 7, 64])
def test_pendulum_quantiles_are_nearest_ranks_of_the_particles(L, P):
    B, Hq = 3, 5
    rng = np.random.default_rng(P)
    states = np.ascontiguousarray(O.pendulum_start_states(B), F)
    seq = rng.uniform(-2, 2, (B, Hq, 1)).astype(F)
    eps = rng.standard_normal((B, P, Hq, 3)).astype(F)
    eng = _engine(L, L.OPT_NONE, 2, 3)
    eng.set_particles(P, AGG_SIGMA, 0.0)
    ranks = [0, P // 2, P - 1]
    out = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True, quantile_ranks=ranks)
    assert [o.shape for o in out] == [(B, Hq, 3), (B, Hq, 3), (B, Hq), (B, Hq), (B, 3, Hq, 3), (B, 3, Hq), (B, P, Hq, 3), (B, P, Hq)]
    _check_quantiles(out, ranks, P)
    plain = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)
    for a, b in zip(out[:4] + out[6:], plain):                  # moments and particles: the other entry point's bits
        np.testing.assert_array_equal(a, b)
    if P == 1:
        np.testing.assert_array_equal(out[4][:, 0], out[6][:, 0])


def test_mlp_quantiles_scratch_and_ties(L):
    B, Hq, P = 3, 3, 4
    eng = _tiny_mlp(L, 2, 3, members=2)
    rng = np.random.default_rng(8)
    states = np.ascontiguousarray(O.pendulum_start_states(B), F)
    seq = rng.uniform(-1, 1, (B, Hq, 1)).astype(F)
    eps = rng.standard_normal((B, P, Hq, 3)).astype(F)
    eng.set_particles(P, np.full(3, 0.02, F), 0.0)
    ranks = [0, 2, 3]
    out = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True, quantile_ranks=ranks)
    _check_quantiles(out, ranks, P)
    plain = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)
    for a, b in zip(out[:4] + out[6:], plain):
        np.testing.assert_array_equal(a, b)
    # without the particle outputs the rollout writes to the handle's scratch: the same quantiles
    lean = eng.predict_trajectory_particles(states, seq, eps=eps, quantile_ranks=ranks)
    assert len(lean) == 6
    for a, b in zip(lean, out[:6]):
        np.testing.assert_array_equal(a, b)
    # only the quantile outputs
    sq, rq = np.full_like(out[4], np.nan), np.full_like(out[5], np.nan)
    r32 = np.asarray(ranks, np.int32)
    L.check(L.lib.bbmpc_predict_trajectory_quantiles(eng._h, L.ptr(states), L.ptr(seq), B, Hq, L.ptr(eps), None, None, None, None, None, None,
                                                     3, r32.ctypes.data, L.ptr(sq), L.ptr(rq)))
    np.testing.assert_array_equal(sq, out[4])
    np.testing.assert_array_equal(rq, out[5])
    # designed ties: no ensemble and sigma = 0, so the four particles are equal; every rank gives the particle value
    eng.set_mlp_ensemble([])
    eng.set_particles(P, np.zeros(3, F), 0.0)
    tied = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True, quantile_ranks=[0, 1, 2, 3])
    assert np.all(tied[6] == tied[6][:, :1])
    for l in range(4):
        np.testing.assert_array_equal(tied[4][:, l], tied[6][:, 0])
        np.testing.assert_array_equal(tied[5][:, l], tied[7][:, 0])


def test_quantiles_through_the_evaluator_and_the_policy(L):
    pol, _ = _policy("CEM", 0.4, P=20)
    ev = pol._optimizer._trajectory_evaluator
    obs = O.pendulum_start_states(2)
    pol.keep_plan(True)
    pol.act(obs, 0)
    plain = pol.plan_distribution(obs)
    out = pol.plan_distribution(obs, quantiles=[0.05, 0.95])
    assert len(plain) == 5 and len(out) == 7 and out[5].shape == (2, 2, 5, 3) and out[6].shape == (2, 2, 5)
    for a, b in zip(out[:5], plain):
        np.testing.assert_array_equal(a, b)
    assert np.all(out[5][:, 0] <= out[5][:, 1]) and np.all(out[6][:, 0] <= out[6][:, 1])
    one = pol.plan_distribution(obs[0], quantiles=[0.05, 0.95])
    np.testing.assert_array_equal(one[5], out[5][0])
    seq = out[0]
    full = ev.predict_trajectory_distribution(obs, seq, return_particles=True, quantiles=[0.05, 0.5, 1.0])
    assert len(full) == 8 and len(ev.predict_trajectory_distribution(obs, seq)) == 4
    np.testing.assert_array_equal(full[4], RU.nearest_rank(full[6], [0, 9, 19], 1))
    with pytest.raises(ValueError):
        ev.predict_trajectory_distribution(obs, seq, quantiles=[0.0])


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_refusals(L):
    N, A, P, H = 9, 1, 5, 4
    states, seq, eps = pendulum_case(N, A, P, H)
    eng = _engine(L, L.OPT_NONE, A, H)

    def risk(kind, k):
        return L.lib.bbmpc_set_particle_risk(eng._h, kind, k)
    # particles off: kind and range are checked, the rule against P waits for bbmpc_set_particles
    assert risk(2, 1) == L.E_INVALID and risk(-1, 0) == L.E_INVALID
    assert risk(L.RISK_MEAN_STD, 1) == L.E_INVALID and risk(L.RISK_CVAR, 0) == L.E_INVALID and risk(L.RISK_CVAR, 65) == L.E_INVALID
    assert risk(L.RISK_CVAR, 6) == 0
    with pytest.raises(L.BBMPCError) as ei:                     # k > P from bbmpc_set_particles, which names both numbers
        eng.set_particles(P, AGG_SIGMA, 0.0)
    assert ei.value.code == L.E_INVALID and "5" in str(ei.value) and "6" in str(ei.value)
    assert getattr(eng, "P", 0) == 0
    assert risk(L.RISK_CVAR, 2) == 0
    eng.set_particles(P, AGG_SIGMA, 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    before = eng.evaluate_particles(states, seq)
    np.testing.assert_array_equal(before[0], RU.cvar32(before[1], 2))
    # particles on: every refused call leaves the rule as it was
    for kind, k in ((2, 1), (L.RISK_CVAR, 0), (L.RISK_CVAR, 6), (L.RISK_CVAR, -1), (L.RISK_MEAN_STD, 2)):
        assert risk(kind, k) == L.E_INVALID
        after = eng.evaluate_particles(states, seq)
        np.testing.assert_array_equal(after[0], before[0])
        np.testing.assert_array_equal(after[1], before[1])
    assert risk(L.RISK_CVAR, 6) == L.E_INVALID and b"6" in L.lib.bbmpc_last_error() and b"5" in L.lib.bbmpc_last_error()
    eng.set_particles(0)                                        # leaves the rule alone
    eng.set_particles(P, AGG_SIGMA, 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    np.testing.assert_array_equal(eng.evaluate_particles(states, seq)[0], before[0])

    # quantiles
    B, Hq = 3, 5
    st, sq_ = np.ascontiguousarray(O.pendulum_start_states(B), F), np.zeros((B, Hq, 1), F)
    buf = np.zeros(B * 8 * Hq * 3, F)

    def quant(nl, ranks, outs=(0, 0, 0, 0, 0, 0, 1, 1), batch=B, hq=Hq, e=eng):
        r = None if ranks is None else np.asarray(ranks, np.int32)
        return L.lib.bbmpc_predict_trajectory_quantiles(e._h, L.ptr(st), L.ptr(sq_), batch, hq, None,
                                                        *[L.ptr(buf) if o else None for o in outs[:6]], nl,
                                                        None if r is None else r.ctypes.data, *[L.ptr(buf) if o else None for o in outs[6:]])
    assert quant(2, [0, 4]) == 0
    assert quant(0, [0]) == L.E_INVALID and quant(9, [0] * 9) == L.E_INVALID
    assert quant(1, [-1]) == L.E_INVALID and quant(1, [P]) == L.E_INVALID and quant(2, [0, P]) == L.E_INVALID
    assert quant(1, None) == L.E_INVALID
    assert quant(1, [0], outs=(0,) * 8) == L.E_INVALID
    assert quant(1, [0], batch=0) == L.E_INVALID and quant(1, [0], hq=4097) == L.E_INVALID
    # sizes are refused before anything is allocated or read: B * L * Hq * S >= 2^31 while B * P * Hq * S is below
    eng.set_particles(4, AGG_SIGMA, 0.0)
    big = 2 ** 31 // (8 * 4096 * 3) + 1
    assert quant(8, [0] * 8, batch=big, hq=4096) == L.E_UNSUPPORTED
    assert L.lib.bbmpc_predict_trajectory_quantiles_dev(eng._h, 1, 1, big, 4096, None, None, None, None, None, None, None, 8,
                                                        np.zeros(8, np.int32).ctypes.data, 1, None) == L.E_UNSUPPORTED
    with pytest.raises(ValueError):
        eng.predict_trajectory_particles(st, sq_, quantile_ranks=[0] * 9)
    eng.set_particles(0)
    assert quant(1, [0]) == L.E_STATE and b"bbmpc_set_particles" in L.lib.bbmpc_last_error()
