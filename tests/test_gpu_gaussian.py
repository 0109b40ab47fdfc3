"""Learned-variance (Gaussian) heads on the GPU (include/bbmpc.h: bbmpc_set_mlp_logvar_head): per-particle returns against
the NumPy statement of tests/gaussian_util.py with injected noise, zero noise against the handle without heads, the
head -> member assignment, the deterministic paths, the optimizers in lock-step with the oracle's, sharding, refusals, the
Python classes and the NLL fit on the device against the host's."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import gaussian_util as GU
from tests.parity_util import assert_cheetah_rewards
from tests.test_ensemble_cpu import member_evaluators, network
from tests.test_gaussian_cpu import CASES, gaussian_case, gaussian_margin, logvar_bounds, member_heads
from tests.test_particles_cpu import AGG_SIGMA, R_ATOL, R_RTOL

pytestmark = pytest.mark.gpu

F = np.float32
GAUSS, ENS, PART = "k_rollout_mlp_particles_gauss", "k_rollout_mlp_particles_ens", "k_rollout_mlp_particles"


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device visible"
    return _lib


def _engine(L, spec, params, stats, A, H, opt=None, N=0, iters=0, k=0, **kw):
    """tests/test_gpu_mlp._problem's handle with member 0 installed as the model (bbmpc_set_mlp); no ensemble, no heads yet."""
    from blackbox_mpc_amd.engine import Engine
    from tests.test_gpu_activations import CODE
    dims, acts, S, U, reward = spec
    rk = L.REW_CHEETAH if reward == "cheetah" else L.REW_PENDULUM
    eng = Engine(opt if opt is not None else L.OPT_NONE, L.DYN_MLP, rk, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=A,
                 planning_horizon=H, population_size=N, max_iterations=iters, num_elite=k, **kw)
    eng.set_mlp(params[0][0], params[0][1], [CODE[a] for a in acts], stats)
    return eng


def _install(eng, params, raw_heads, bounds):
    """The call order of the ABI: the members (when there are several), then one head per member."""
    if len(params) > 1:
        eng.set_mlp_ensemble(params)
    eng.set_mlp_logvar_head(raw_heads, *bounds)


def _pend(L, E, A, H, **kw):
    spec = network("PEND_MLP")
    params, stats, evs = member_evaluators(spec, E)
    raw, bounds, heads = member_heads(spec, evs)
    return _engine(L, spec, params, stats, A, H, **kw), params, stats, evs, raw, bounds, heads


def _inputs(A, N, H, P, seed):
    rng = np.random.default_rng(seed)
    return (O.pendulum_start_states(A).astype(F), rng.uniform(-1, 1, (N, A, H, 1)).astype(F),
            rng.standard_normal((A, P, H, 3)).astype(F))


# ---- 1. per-particle returns, injected eps --------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)))
def test_returns_match_the_helper(L, case):
    c = gaussian_case(case)
    N, A, P, E, H = c["shape"]
    reward = c["spec"][4]
    assert (c["stats"] is None) == (not CASES[case][7])
    eng = _engine(L, c["spec"], c["params"], c["stats"], A, H)
    eng.set_particles(P, c["sigma"], 0.0)
    _install(eng, c["params"], c["raw_heads"], c["bounds"])
    eng.inject_noise(L.NOISE_PROCESS, c["eps"])
    eng.set_profiling(True)
    scores, got = eng.evaluate_particles(c["states"], c["seq"])
    assert eng.get_profile()[2] == GAUSS
    want = c["want"]
    assert got.shape == (N, P, A) and np.all(np.isfinite(want))
    print("[gaussian case %d] max |dev - helper| = %.3e" % (case, np.abs(got.astype(np.float64) - want).max()))
    if reward == "cheetah":
        assert_cheetah_rewards(got.reshape(N * P, A), want.reshape(N * P, A), 1e-3, 1e-3 * H,
                               margin=lambda: gaussian_margin(case).reshape(N * P, A))
    else:
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)
    np.testing.assert_array_equal(eng.evaluate(c["states"], c["seq"]), scores)


# ---- 2. eps = 0 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2])
def test_zero_noise_is_the_handle_without_heads_bit_for_bit(L, E):
    spec = network("CHEETAH")
    N, A, P, H = 37, 3, 4, 12
    params, stats, evs = member_evaluators(spec, E)
    raw, bounds, _ = member_heads(spec, evs)
    eng = _engine(L, spec, params, stats, A, H)
    rng = np.random.default_rng(8)
    states = O.cheetah_start_states(A, 20).astype(F)
    seq = rng.uniform(-1, 1, (N, A, H, 6)).astype(F)
    eng.set_particles(P, np.full(20, 0.02, F), 1.5)                         # sigma != 0
    if E > 1:
        eng.set_mlp_ensemble(params)
    eng.inject_noise(L.NOISE_PROCESS, np.zeros((A, P, H, 20), F))
    eng.set_profiling(True)
    s0, r0 = eng.evaluate_particles(states, seq)
    assert eng.get_profile()[2] == (ENS if E > 1 else PART)
    eng.set_mlp_logvar_head(raw, *bounds)
    s1, r1 = eng.evaluate_particles(states, seq)
    assert eng.get_profile()[2] == GAUSS
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(s1, s0)
    eng.set_mlp_logvar_head([])                                             # num_heads = 0 removes them
    s2, r2 = eng.evaluate_particles(states, seq)
    assert eng.get_profile()[2] == (ENS if E > 1 else PART)
    np.testing.assert_array_equal(r2, r0)
    assert np.all(np.isfinite(r0)) and np.any(r0[0] != r0[1])
    # ... and with noise the heads do change the returns
    eng.set_mlp_logvar_head(raw, *bounds)
    eng.inject_noise(L.NOISE_PROCESS, rng.standard_normal((A, P, H, 20)).astype(F))
    assert not np.array_equal(eng.evaluate_particles(states, seq)[1], r0)


# ---- 3. which head follows which member ------------------------------------------------------------------------------
def test_head_e_follows_member_e(L):
    """Two members with the SAME mean network and constant heads (zero kernel): member 0's sd is e^-10 std_t, member 1's
    e^-1.5 std_t, sigma = 0.  Against the noise-free returns, the particles of member 0 (p even) barely move for any
    candidate and those of member 1 (p odd) move for every candidate."""
    N, A, P, E, H = 21, 2, 4, 2, 5
    eng, params, stats, evs, _, _, _ = _pend(L, 1, A, H)
    states, seq, eps = _inputs(A, N, H, P, 3)
    zero_w = np.zeros((32, 3), F)
    heads = [(zero_w, np.full(3, -30.0, F)), (zero_w, np.full(3, -3.0, F))]
    lo, hi = np.full(3, -20.0, F), np.full(3, 0.0, F)
    eng.set_mlp_ensemble([params[0], params[0]])
    eng.set_mlp_logvar_head(heads, lo, hi)
    eng.set_particles(P, np.zeros(3, F), 0.0)
    eng.inject_noise(L.NOISE_PROCESS, np.zeros_like(eps))
    _, quiet = eng.evaluate_particles(states, seq)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    _, r = eng.evaluate_particles(states, seq)
    move = np.abs(r.astype(np.float64) - quiet)
    print("max move of member 0's particles %.3e, min move of member 1's %.3e" % (move[:, 0::2].max(), move[:, 1::2].min()))
    assert move[:, 0::2].max() < 1e-2 < move[:, 1::2].min()
    h0, h1 = GU.Head(evs[0], *heads[0], lo, hi), GU.Head(evs[0], *heads[1], lo, hi)
    want = GU.gaussian_particle_returns([evs[0], evs[0]], [h0, h1], states, seq, eps, np.zeros(3, F), P)
    np.testing.assert_allclose(r, want, rtol=1e-3, atol=1e-3 * H)
    # swapped heads swap the roles
    eng.set_mlp_logvar_head(heads[::-1], lo, hi)
    move = np.abs(eng.evaluate_particles(states, seq)[1].astype(np.float64) - quiet)
    assert move[:, 1::2].max() < 1e-2 < move[:, 0::2].min()


# ---- 4. the deterministic paths --------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2])
def test_deterministic_paths_are_unchanged_by_installing_heads(L, E):
    N, A, H, iters, k, P = 64, 2, 8, 2, 8, 4
    eng, params, stats, evs, raw, bounds, _ = _pend(L, E, A, H, opt=L.OPT_CEM, N=N, iters=iters, k=k)
    rng = np.random.default_rng(2)
    trunc = np.stack([O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)])
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, trunc)
    states = O.pendulum_start_states(A).astype(F)
    act = rng.uniform(-1, 1, (A, 1)).astype(F)
    seq = rng.uniform(-1, 1, (9, A, H, 1)).astype(F)
    if E > 1:
        eng.set_mlp_ensemble(params)

    def snapshot():
        return (eng.predict_next_state(states, act), *eng.predict_trajectories(states, seq[0]), eng.evaluate(states, seq),
                *eng.optimize(states))
    before = snapshot()
    eng.set_mlp_logvar_head(raw, *bounds)
    for x, y in zip(snapshot(), before):
        np.testing.assert_array_equal(x, y)
    # with particles on the heads take part in the scores, the record stays the mean network's one-step prediction
    eng.set_particles(P, AGG_SIGMA, 1.0)
    a1, n1, _ = eng.optimize(states)
    np.testing.assert_allclose(n1, eng.predict_next_state(states, a1), rtol=2e-5, atol=2e-5)
    eng.set_particles(0)
    for x, y in zip(snapshot(), before):
        np.testing.assert_array_equal(x, y)


# ---- 5. optimizers, injected draws ----------------------------------------------------------------------------------
def test_random_search_lockstep(L):
    N, A, H, P, E = 64, 2, 8, 4, 2
    eng, params, stats, evs, raw, bounds, heads = _pend(L, E, A, H, opt=L.OPT_RANDOM_SEARCH, N=N)
    rng = np.random.default_rng(5)
    eps = rng.standard_normal((1, A, P, H, 3)).astype(F)
    u01 = rng.random((N, A, H, 1)).astype(F)
    eng.set_trace(True)
    _install(eng, params, raw, bounds)
    eng.set_particles(P, AGG_SIGMA, 1.0)
    eng.inject_noise(L.NOISE_UNIFORM, u01)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    rs = O.RandomSearch(GU.GaussianParticleEvaluator(evs, heads, P, AGG_SIGMA, 1.0, eps), [-1.0], [1.0], horizon=H, population=N,
                        num_agents=A)
    act_o, nxt_o, rew_o = rs.call(states, {"uniform": u01})
    np.testing.assert_array_equal(eng.get_trace(0, L.TRACE_SAMPLES), rs.trace[0]["samples"])
    np.testing.assert_allclose(eng.get_trace(0, L.TRACE_REWARDS), rs.trace[0]["rewards"], rtol=R_RTOL, atol=R_ATOL)
    np.testing.assert_array_equal(eng.get_trace(0, L.TRACE_ELITES), rs.trace[0]["best"])
    np.testing.assert_array_equal(act, act_o)
    np.testing.assert_allclose(nxt, nxt_o, rtol=2e-5, atol=2e-5)             # the record: member 0's mean network, no noise
    np.testing.assert_allclose(rew, rew_o, rtol=1e-4, atol=1e-3)


def test_cem_lockstep(L):
    N, A, H, iters, k, P, E = 64, 1, 8, 3, 8, 4, 2
    eng, params, stats, evs, raw, bounds, heads = _pend(L, E, A, H, opt=L.OPT_CEM, N=N, iters=iters, k=k)
    rng = np.random.default_rng(17)
    eps = rng.standard_normal((iters, A, P, H, 3)).astype(F)
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]}
    eng.set_trace(True)
    _install(eng, params, raw, bounds)
    eng.set_particles(P, AGG_SIGMA, 0.5)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    eng.inject_noise(L.NOISE_PROCESS, eps)
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    hip_el = [eng.get_trace(it, L.TRACE_ELITES) for it in range(iters)]
    hip_r = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(iters)]

    def select(it, r_o, own):                            # the forced-elites hook of tests/test_gpu_particles.py
        np.testing.assert_allclose(hip_r[it], r_o, rtol=R_RTOL, atol=R_ATOL)
        for a in range(A):
            he = hip_el[it][a]
            if set(own[a]) != set(he):
                kth = np.sort(r_o[:, a])[::-1][k - 1]
                for n in set(own[a]) ^ set(he):
                    assert abs(r_o[n, a] - kth) <= R_ATOL + R_RTOL * abs(kth)
            np.testing.assert_array_equal(he, O.topk_desc(hip_r[it][:, a], k))
        return hip_el[it]
    cem = O.CEM(GU.GaussianParticleEvaluator(evs, heads, P, AGG_SIGMA, 0.5, eps), [-1.0], [1.0], horizon=H, max_iterations=iters,
                population=N, num_elite=k, num_agents=A)
    cem._optimize(states, noise, forced_elites=select)
    for it in range(iters):
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_SAMPLES), cem.trace[it]["samples"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), cem.trace[it]["mean"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_VAR), cem.trace[it]["var"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(act, cem.trace[-1]["mean"][:, 0], rtol=0, atol=2e-5)


# ---- 6. sharding ----------------------------------------------------------------------------------------------------
def test_agent_sharding_is_bit_identical(L):
    N, A, P, E, H = 40, 2, 4, 2, 7
    states, seq, _ = _inputs(A, N, H, P, 6)
    whole, params, stats, _, raw, bounds, _ = _pend(L, E, A, H, seed=99)
    _install(whole, params, raw, bounds)
    whole.set_particles(P, AGG_SIGMA, 1.5)
    want = whole.evaluate(states, seq)
    for a in range(A):
        shard = _pend(L, E, 1, H, seed=99, agent_offset=a, num_agents_global=A)[0]
        _install(shard, params, raw, bounds)
        shard.set_particles(P, AGG_SIGMA, 1.5)
        np.testing.assert_array_equal(shard.evaluate(states[a:a + 1], seq[:, a:a + 1])[:, 0], want[:, a])
    assert np.any(want[:, 0] != want[:, 1])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(L):
    from blackbox_mpc_amd.engine import Engine
    N, A, H = 9, 1, 5
    states, seq, _ = _inputs(A, N, H, 4, 7)
    sigma = np.full(3, 0.1, F)
    eng, params, stats, _, raw, bounds, _ = _pend(L, 2, A, H)
    eng.set_particles(4, sigma, 1.0)
    eng.set_mlp_ensemble(params)
    ens = eng.evaluate(states, seq)
    # a wrong num_heads: one head for two members, three for two; the message names both numbers
    for heads, n in ((raw[:1], "1"), (raw + raw[:1], "3")):
        with pytest.raises(L.BBMPCError) as ei:
            eng.set_mlp_logvar_head(heads, *bounds)
        assert ei.value.code == L.E_INVALID and n in str(ei.value) and "2" in str(ei.value)
        np.testing.assert_array_equal(eng.evaluate(states, seq), ens)
    eng.set_mlp_logvar_head(raw, *bounds)
    gauss = eng.evaluate(states, seq)
    assert not np.array_equal(gauss, ens)
    # bad bounds: min > max, outside [-40, 40], not finite -- the installed heads stay
    lo, hi = bounds
    for blo, bhi in ((hi, lo), (lo - F(40), hi), (lo, hi + F(50)), (np.full(3, np.nan, F), hi), (lo, np.full(3, np.inf, F))):
        with pytest.raises(L.BBMPCError) as ei:
            eng.set_mlp_logvar_head(raw, blo, bhi)
        assert ei.value.code == L.E_INVALID
        np.testing.assert_array_equal(eng.evaluate(states, seq), gauss)
    # null pointers
    null = (ctypes.c_void_p * 2)()
    wp = (ctypes.c_void_p * 2)(*[w.ctypes.data for w, _ in raw])
    assert L.lib.bbmpc_set_mlp_logvar_head(eng._h, 2, None, None, None, None) == L.E_INVALID
    assert L.lib.bbmpc_set_mlp_logvar_head(eng._h, 2, wp, null, lo.ctypes.data, hi.ctypes.data) == L.E_INVALID
    np.testing.assert_array_equal(eng.evaluate(states, seq), gauss)
    # heads vanish after bbmpc_set_mlp_ensemble (also with num_members = 0) and after bbmpc_set_mlp
    eng.set_profiling(True)
    eng.set_mlp_ensemble(params)
    np.testing.assert_array_equal(eng.evaluate(states, seq), ens)
    assert eng.get_profile()[2] == ENS
    eng.set_mlp_logvar_head(raw, *bounds)
    eng.set_mlp_ensemble([])
    single = eng.evaluate(states, seq)
    assert eng.get_profile()[2] == PART
    eng.set_mlp_logvar_head(raw[:1], *bounds)                               # one model now: one head
    one = eng.evaluate(states, seq)
    assert eng.get_profile()[2] == GAUSS and not np.array_equal(one, single)
    eng.set_mlp(params[0][0], params[0][1], [1, 1, 1, 0], stats)
    np.testing.assert_array_equal(eng.evaluate(states, seq), single)
    assert eng.get_profile()[2] == PART
    # before bbmpc_set_mlp; on a handle that is not BBMPC_DYN_MLP
    fresh = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-1.0], [1.0], dim_s=3, num_agents=A, planning_horizon=H)
    with pytest.raises(L.BBMPCError) as ei:
        fresh.set_mlp_logvar_head(raw[:1], *bounds)
    assert ei.value.code == L.E_STATE
    fresh.set_mlp(params[0][0], params[0][1], [1, 1, 1, 0], stats)
    fresh.set_particles(4, sigma, 1.0)
    np.testing.assert_array_equal(fresh.evaluate(states, seq), single)
    fresh.set_mlp_logvar_head(raw[:1], *bounds)
    np.testing.assert_array_equal(fresh.evaluate(states, seq), one)
    pend = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-1.0], [1.0], dim_s=3, num_agents=A, planning_horizon=H)
    want = pend.evaluate(states, seq)
    with pytest.raises(L.BBMPCError) as ei:
        pend.set_mlp_logvar_head(raw[:1], *bounds)
    assert ei.value.code == L.E_STATE
    np.testing.assert_array_equal(pend.evaluate(states, seq), want)
    # the Python wrapper refuses a kernel that does not sit on the last hidden layer
    with pytest.raises(ValueError):
        fresh.set_mlp_logvar_head([(np.zeros((31, 3), F), np.zeros(3, F))], *bounds)


# ---- 8. Python ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [0, 2])
def test_mpc_policy_with_probabilistic_models_and_the_particle_evaluator(L, members):
    from blackbox_mpc_amd.dynamics_functions import EnsembleMLP, ProbabilisticMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.trajectory_evaluators import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    from tests.test_gpu_mlp import _stats
    act_space, obs_space = Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8])
    layers, acts = [4, 32, 32, 3], ["tanh", "tanh", None]
    if members:
        fn = EnsembleMLP(layers, acts, num_members=members, seed=9, probabilistic=True, min_logvar=-8.0, max_logvar=-2.0)
        models = fn.members
    else:
        fn = ProbabilisticMLP(layers, acts, min_logvar=-8.0, max_logvar=-2.0, seed=9)
        models = [fn]
    for m in models:                                         # small outputs: the closed loop stays in the pendulum's range
        m.set_weights(m.weights[:-1] + [m.weights[-1] * F(0.1)], m.biases)
        m.set_logvar_head(m.logvar_weights, m.logvar_bias - F(4.0))
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=fn, is_normalized=True)
    stats = _stats(3, 1, 44)
    handler.set_normalization_stats(*stats)
    ev = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=4, process_noise_std=0.0, risk_kappa=1.0)
    pol = MPCPolicy(trajectory_evaluator=ev, env_action_space=act_space, env_observation_space=obs_space,
                    optimizer_name="CEM", num_agents=1, planning_horizon=8, population_size=64, max_iterations=2,
                    num_elite=8, seed=11)

    def direct(heads, **kw):
        kw = kw or dict(opt=L.OPT_CEM, population_size=64, max_iterations=2, num_elite=8, seed=11)
        eng = Engine(kw.pop("opt", L.OPT_NONE), L.DYN_MLP, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=8, **kw)
        eng.set_mlp(fn.weights, fn.biases, fn.activation_codes, stats)
        if members:
            eng.set_mlp_ensemble(models)
        if heads:
            eng.set_mlp_logvar_head(models, fn.min_logvar, fn.max_logvar)
        eng.set_particles(4, np.zeros(3, F), 1.0)
        return eng
    eng, headless = direct(True), direct(False)
    obs = np.array([1.0, 0.0, 0.0], F)
    differs = False
    for t in range(5):
        a, n, r = pol.act(obs, t)
        a_e, n_e, r_e = eng.optimize(obs[None])
        np.testing.assert_array_equal(a, a_e[0])
        np.testing.assert_array_equal(n, n_e[0])
        np.testing.assert_array_equal(r, r_e[0])
        differs = differs or not np.array_equal(a_e, headless.optimize(obs[None])[0])
        obs = n.astype(F)
    assert differs                                           # at sigma = 0 the learned noise alone moves the policy's scores
    seq = np.random.default_rng(3).uniform(-2, 2, (9, 1, 8, 1)).astype(F)
    returns = ev.particle_returns(obs[None], seq)
    assert returns.shape == (9, 4, 1) and ev(obs[None], seq).shape == (9, 1)
    np.testing.assert_array_equal(returns, direct(True, opt=L.OPT_NONE).evaluate_particles(obs[None], seq)[1])
    assert np.all(np.ptp(returns, axis=1) > 0)               # spread from the head alone
    # a refit of one head alone reaches the engines (the function's version bumps)
    models[-1].set_logvar_head(models[-1].logvar_weights, models[-1].logvar_bias + F(2.0))
    again = ev.particle_returns(obs[None], seq)
    assert not np.array_equal(again, returns)
    np.testing.assert_array_equal(again, direct(True, opt=L.OPT_NONE).evaluate_particles(obs[None], seq)[1])


# ---- 9. the NLL fit on the device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"])
def test_gpu_nll_training_matches_the_host_trainer(L, monkeypatch, graph):
    """tests/test_gpu_train.py's comparison (parameters atol 3e-4, losses rtol 2e-4 / atol 1e-6), the reference being the
    same DenseTrainer.fit on the host."""
    from blackbox_mpc_amd.dynamics_functions import ProbabilisticMLP
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer
    monkeypatch.setenv("BBMPC_TRAIN_GRAPH", graph)
    rng = np.random.default_rng(4)
    n, epochs, B = 480, 6, 32
    x = rng.normal(0, 1, (n, 4)).astype(F)
    y = (np.tanh(x[:, :3]) * 0.5 + (0.05 + 0.2 * (x[:, 3:] > 0)) * rng.standard_normal((n, 3))).astype(F)
    perms = [rng.permutation(n - 96) for _ in range(epochs)]
    fn = ProbabilisticMLP([4, 64, 64, 3], ["tanh", "tanh", None], seed=3)
    out = {}
    for dev in ("cuda", "cpu"):
        tr = DenseTrainer(fn.weights, fn.biases, fn.activation_codes, dev, learning_rate=2e-3,
                          logvar_head=(fn.logvar_weights, fn.logvar_bias, fn.min_logvar, fn.max_logvar))
        tl, vl = tr.fit(x[96:], y[96:], x[:96], y[:96], epochs, B, permutations=perms)
        assert (tr._graph is not None) == (dev == "cuda" and graph == "1")
        ws, bs = tr.numpy_params()
        out[dev] = (ws + bs + list(tr.numpy_logvar_head()), tl, vl)
    for got, want in zip(out["cuda"][0], out["cpu"][0]):
        np.testing.assert_allclose(got, want, rtol=0, atol=3e-4)
    assert not np.array_equal(out["cuda"][0][-2], fn.logvar_weights)
    np.testing.assert_allclose(out["cuda"][1], out["cpu"][1], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(out["cuda"][2], out["cpu"][2], rtol=2e-4, atol=1e-6)
    assert out["cpu"][1][-1] < out["cpu"][1][0]
