"""Model ensembles with trajectory sampling on the GPU (include/bbmpc.h: bbmpc_set_mlp_ensemble): per-particle returns
against the NumPy statement of tests/ensemble_util.py with injected noise, identical members against the single-model
path, the particle -> member assignment, the primary on the deterministic paths, the optimizers in lock-step with the
oracle's, sharding, refusals and the Python classes."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import ensemble_util as EU
from tests.parity_util import assert_cheetah_rewards
from tests.test_ensemble_cpu import CASES, ensemble_case, ensemble_margin, member_evaluators, network
from tests.test_particles_cpu import AGG_SIGMA, R_ATOL, R_RTOL

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device visible"
    return _lib


def _engine(L, spec, params, stats, A, H, opt=None, N=0, iters=0, k=0, **kw):
    """tests/test_gpu_mlp._problem's handle with member 0 installed as the model (bbmpc_set_mlp); no ensemble yet."""
    from blackbox_mpc_amd.engine import Engine
    from tests.test_gpu_activations import CODE
    dims, acts, S, U, reward = spec
    rk = L.REW_CHEETAH if reward == "cheetah" else L.REW_PENDULUM
    eng = Engine(opt if opt is not None else L.OPT_NONE, L.DYN_MLP, rk, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=A,
                 planning_horizon=H, population_size=N, max_iterations=iters, num_elite=k, **kw)
    eng.set_mlp(params[0][0], params[0][1], [CODE[a] for a in acts], stats)
    return eng


def _pend(L, E, A, H, **kw):
    spec = network("PEND_MLP")
    params, stats, evs = member_evaluators(spec, E)
    return _engine(L, spec, params, stats, A, H, **kw), params, stats, evs


def _inputs(A, N, H, P, seed):
    rng = np.random.default_rng(seed)
    return (O.pendulum_start_states(A).astype(F), rng.uniform(-1, 1, (N, A, H, 1)).astype(F),
            rng.standard_normal((A, P, H, 3)).astype(F))


# ---- 1. per-particle returns, injected eps --------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)))
def test_returns_match_the_helper(L, case):
    c = ensemble_case(case)
    N, A, P, E, H = c["shape"]
    reward = c["spec"][4]
    eng = _engine(L, c["spec"], c["params"], c["stats"], A, H)
    eng.set_particles(P, c["sigma"], 0.0)
    eng.set_mlp_ensemble(c["params"])
    eng.inject_noise(L.NOISE_PROCESS, c["eps"])
    eng.set_profiling(True)
    scores, got = eng.evaluate_particles(c["states"], c["seq"])
    assert eng.get_profile()[2] == "k_rollout_mlp_particles_ens"
    want = c["want"]
    assert got.shape == (N, P, A) and np.all(np.isfinite(want))
    print("[ensemble case %d] max |dev - helper| = %.3e" % (case, np.abs(got.astype(np.float64) - want).max()))
    if reward == "cheetah":
        # row order (n, p) of both arrays; the margin is the helper's own (tests/test_ensemble_cpu.py: no row is near a threshold)
        assert_cheetah_rewards(got.reshape(N * P, A), want.reshape(N * P, A), 1e-3, 1e-3 * H,
                               margin=lambda: ensemble_margin(case).reshape(N * P, A))
    else:
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)
    np.testing.assert_array_equal(eng.evaluate(c["states"], c["seq"]), scores)


# ---- 2. identical members -------------------------------------------------------------------------------------------
def test_identical_members_are_the_single_model_path_bit_for_bit(L):
    spec = network("CHEETAH")
    N, A, P, H = 37, 3, 4, 12
    params, stats, _ = member_evaluators(spec, 1)
    eng = _engine(L, spec, params, stats, A, H)
    rng = np.random.default_rng(8)
    states = O.cheetah_start_states(A, 20).astype(F)
    seq = rng.uniform(-1, 1, (N, A, H, 6)).astype(F)
    eng.set_particles(P, np.full(20, 0.02, F), 1.5)
    eng.inject_noise(L.NOISE_PROCESS, rng.standard_normal((A, P, H, 20)).astype(F))
    eng.set_profiling(True)
    s0, r0 = eng.evaluate_particles(states, seq)
    assert eng.get_profile()[2] == "k_rollout_mlp_particles"
    eng.set_mlp_ensemble([params[0], params[0]])
    s1, r1 = eng.evaluate_particles(states, seq)
    assert eng.get_profile()[2] == "k_rollout_mlp_particles_ens"
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(s1, s0)
    eng.set_mlp_ensemble([])
    s2, r2 = eng.evaluate_particles(states, seq)
    assert eng.get_profile()[2] == "k_rollout_mlp_particles"
    np.testing.assert_array_equal(r2, r0)
    np.testing.assert_array_equal(s2, s0)
    assert np.all(np.isfinite(r0)) and np.any(r0[:, 0] != r0[:, 1])


# ---- 3. which particle follows which member ---------------------------------------------------------------------------
def test_particle_p_follows_member_p_mod_E(L):
    N, A, P, E, H = 21, 2, 4, 2, 5
    eng, params, stats, _ = _pend(L, E, A, H)
    bad = ([w.copy() for w in params[1][0]], params[1][1])
    bad[0][-1][3, 1] = np.nan
    states, seq, eps = _inputs(A, N, H, P, 3)
    eng.set_mlp_ensemble([params[0], bad])
    eng.set_particles(P, np.full(3, 0.02, F), 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    _, r = eng.evaluate_particles(states, seq)
    assert np.all(r[:, 1::2] == F(-1e6))
    assert np.all(np.isfinite(r[:, 0::2])) and np.all(r[:, 0::2] > F(-1e5))


# ---- 4. the primary serves the deterministic paths -------------------------------------------------------------------
def test_the_primary_serves_the_deterministic_paths(L):
    N, A, H, iters, k, P, E = 64, 2, 8, 2, 8, 4, 2
    eng, params, stats, evs = _pend(L, E, A, H, opt=L.OPT_CEM, N=N, iters=iters, k=k)
    plain = _engine(L, network("PEND_MLP"), params, stats, A, H, opt=L.OPT_CEM, N=N, iters=iters, k=k)
    other = _engine(L, network("PEND_MLP"), params[1:], stats, A, H)                  # member 1 as a handle's model
    rng = np.random.default_rng(2)
    trunc = np.stack([O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)])
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, trunc)
    plain.inject_noise(L.NOISE_TRUNC_NORMAL, trunc)
    states = O.pendulum_start_states(A).astype(F)
    eng.set_mlp_ensemble(params)
    eng.set_particles(P, AGG_SIGMA, 1.0)
    act, nxt, rew = eng.optimize(states)
    # (the record comes from the tail's row code, predict_next_state from the MFMA step kernel: the single-step bound of
    # tests/test_gpu_mlp.py between them, bit-equal answers between the two handles)
    np.testing.assert_allclose(nxt, eng.predict_next_state(states, act), rtol=2e-5, atol=2e-5)
    np.testing.assert_array_equal(eng.predict_next_state(states, act), plain.predict_next_state(states, act))
    assert np.abs(nxt - other.predict_next_state(states, act)).max() > 1e-3       # (the members do differ at this point)
    np.testing.assert_array_equal(eng.predict_trajectories(states, act[:, None, :])[0],
                                  plain.predict_trajectories(states, act[:, None, :])[0])
    eng.set_particles(0)                                     # CEM restarts from its constructor distribution (quirk Q2)
    for x, y in zip(eng.optimize(states), plain.optimize(states)):
        np.testing.assert_array_equal(x, y)
    seq = rng.uniform(-1, 1, (9, A, H, 1)).astype(F)
    np.testing.assert_array_equal(eng.evaluate(states, seq), plain.evaluate(states, seq))


# ---- 5. optimizers, injected draws ----------------------------------------------------------------------------------
def test_random_search_lockstep(L):
    N, A, H, P, E = 64, 2, 8, 4, 2
    eng, params, stats, evs = _pend(L, E, A, H, opt=L.OPT_RANDOM_SEARCH, N=N)
    rng = np.random.default_rng(5)
    eps = rng.standard_normal((1, A, P, H, 3)).astype(F)
    u01 = rng.random((N, A, H, 1)).astype(F)
    eng.set_trace(True)
    eng.set_mlp_ensemble(params)
    eng.set_particles(P, AGG_SIGMA, 1.0)
    eng.inject_noise(L.NOISE_UNIFORM, u01)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    rs = O.RandomSearch(EU.EnsembleParticleEvaluator(evs, P, AGG_SIGMA, 1.0, eps), [-1.0], [1.0], horizon=H, population=N, num_agents=A)
    act_o, nxt_o, rew_o = rs.call(states, {"uniform": u01})
    np.testing.assert_array_equal(eng.get_trace(0, L.TRACE_SAMPLES), rs.trace[0]["samples"])
    np.testing.assert_allclose(eng.get_trace(0, L.TRACE_REWARDS), rs.trace[0]["rewards"], rtol=R_RTOL, atol=R_ATOL)
    np.testing.assert_array_equal(eng.get_trace(0, L.TRACE_ELITES), rs.trace[0]["best"])
    np.testing.assert_array_equal(act, act_o)
    # the record stays the noise-free one-step prediction of member 0 (the oracle evaluator's handler)
    np.testing.assert_allclose(nxt, nxt_o, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(rew, rew_o, rtol=1e-4, atol=1e-3)


def test_cem_lockstep(L):
    N, A, H, iters, k, P, E = 64, 1, 8, 3, 8, 4, 2
    eng, params, stats, evs = _pend(L, E, A, H, opt=L.OPT_CEM, N=N, iters=iters, k=k)
    rng = np.random.default_rng(17)
    eps = rng.standard_normal((iters, A, P, H, 3)).astype(F)
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]}
    eng.set_trace(True)
    eng.set_mlp_ensemble(params)
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
    cem = O.CEM(EU.EnsembleParticleEvaluator(evs, P, AGG_SIGMA, 0.5, eps), [-1.0], [1.0], horizon=H, max_iterations=iters,
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
    whole, params, stats, _ = _pend(L, E, A, H, seed=99)
    whole.set_mlp_ensemble(params)
    whole.set_particles(P, AGG_SIGMA, 1.5)
    want = whole.evaluate(states, seq)
    for a in range(A):
        shard, _, _, _ = _pend(L, E, 1, H, seed=99, agent_offset=a, num_agents_global=A)
        shard.set_mlp_ensemble(params)
        shard.set_particles(P, AGG_SIGMA, 1.5)
        np.testing.assert_array_equal(shard.evaluate(states[a:a + 1], seq[:, a:a + 1])[:, 0], want[:, a])
    assert np.any(want[:, 0] != want[:, 1])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(L):
    from blackbox_mpc_amd.engine import Engine
    N, A, H = 9, 1, 5
    states, seq, _ = _inputs(A, N, H, 3, 7)
    sigma = np.full(3, 0.1, F)
    eng, params, stats, _ = _pend(L, 3, A, H)
    # num_particles % num_members != 0, the ensemble second ...
    eng.set_particles(3, sigma, 1.0)
    before = eng.evaluate(states, seq)
    with pytest.raises(L.BBMPCError) as ei:
        eng.set_mlp_ensemble(params[:2])
    assert ei.value.code == L.E_INVALID and "3" in str(ei.value) and "2" in str(ei.value)
    np.testing.assert_array_equal(eng.evaluate(states, seq), before)
    # ... and the particles second: the ensemble and the old particle count stay
    eng.set_mlp_ensemble(params)
    ens = eng.evaluate(states, seq)
    assert not np.array_equal(ens, before)
    with pytest.raises(L.BBMPCError) as ei:
        eng.set_particles(4, sigma, 1.0)
    assert ei.value.code == L.E_INVALID and "4" in str(ei.value) and "3" in str(ei.value)
    np.testing.assert_array_equal(eng.evaluate(states, seq), ens)
    # more than eight members; null pointers
    with pytest.raises(L.BBMPCError) as ei:
        eng.set_mlp_ensemble([params[0]] * 9)
    assert ei.value.code == L.E_UNSUPPORTED
    assert L.lib.bbmpc_set_mlp_ensemble(eng._h, 3, None, None) == L.E_INVALID
    assert L.lib.bbmpc_set_mlp_ensemble(eng._h, -1, None, None) == L.E_UNSUPPORTED
    null = (ctypes.c_void_p * 12)()
    assert L.lib.bbmpc_set_mlp_ensemble(eng._h, 3, null, null) == L.E_INVALID
    np.testing.assert_array_equal(eng.evaluate(states, seq), ens)
    # a later bbmpc_set_mlp removes the ensemble
    eng.set_mlp(params[0][0], params[0][1], [1, 1, 1, 0], stats)
    np.testing.assert_array_equal(eng.evaluate(states, seq), before)
    # before bbmpc_set_mlp; on a handle that is not BBMPC_DYN_MLP
    fresh = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-1.0], [1.0], dim_s=3, num_agents=A, planning_horizon=H)
    with pytest.raises(L.BBMPCError) as ei:
        fresh.set_mlp_ensemble(params)
    assert ei.value.code == L.E_STATE
    fresh.set_mlp(params[0][0], params[0][1], [1, 1, 1, 0], stats)
    fresh.set_particles(3, sigma, 1.0)
    np.testing.assert_array_equal(fresh.evaluate(states, seq), before)
    pend = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-1.0], [1.0], dim_s=3, num_agents=A, planning_horizon=H)
    want = pend.evaluate(states, seq)
    with pytest.raises(L.BBMPCError) as ei:
        pend.set_mlp_ensemble(params)
    assert ei.value.code == L.E_STATE
    np.testing.assert_array_equal(pend.evaluate(states, seq), want)


# ---- 8. Python ------------------------------------------------------------------------------------------------------
def test_mpc_policy_with_an_ensemble_and_the_particle_evaluator(L):
    from blackbox_mpc_amd.dynamics_functions import EnsembleMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator, ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    from tests.test_gpu_mlp import _stats
    act_space, obs_space = Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8])
    fn = EnsembleMLP([4, 32, 32, 3], ["tanh", "tanh", None], num_members=2, seed=9)
    for m in fn.members:                                     # small outputs: the closed loop stays in the pendulum's range
        m.set_weights(m.weights[:-1] + [m.weights[-1] * F(0.1)], m.biases)
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=fn, is_normalized=True)
    stats = _stats(3, 1, 44)
    handler.set_normalization_stats(*stats)
    sigma = [0.02, 0.02, 0.2]
    ev = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=4, process_noise_std=sigma, risk_kappa=1.0)
    pol = MPCPolicy(trajectory_evaluator=ev, env_action_space=act_space, env_observation_space=obs_space,
                    optimizer_name="CEM", num_agents=1, planning_horizon=8, population_size=64, max_iterations=2,
                    num_elite=8, seed=11)

    def direct(members):
        eng = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=8,
                     population_size=64, max_iterations=2, num_elite=8, seed=11)
        eng.set_mlp(fn.weights, fn.biases, fn.activation_codes, stats)
        if members:
            eng.set_mlp_ensemble(members)
        eng.set_particles(4, np.array(sigma, F), 1.0)
        return eng
    eng, single = direct(fn.members), direct(None)
    obs = np.array([1.0, 0.0, 0.0], F)
    differs = False
    for t in range(5):
        a, n, r = pol.act(obs, t)
        a_e, n_e, r_e = eng.optimize(obs[None])
        np.testing.assert_array_equal(a, a_e[0])
        np.testing.assert_array_equal(n, n_e[0])
        np.testing.assert_array_equal(r, r_e[0])
        differs = differs or not np.array_equal(a_e, single.optimize(obs[None])[0])
        obs = n.astype(F)
    assert differs                                           # the second member does take part in the policy's scores
    # the evaluator's own calls: member p % 2 behind particle p, member 0 behind the deterministic calls
    seq = np.random.default_rng(3).uniform(-2, 2, (9, 1, 8, 1)).astype(F)
    def fresh(members):                                      # the evaluator's own handle: seed 0, control step 0
        e2 = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=8)
        e2.set_mlp(fn.weights, fn.biases, fn.activation_codes, stats)
        if members:
            e2.set_mlp_ensemble(members)
        e2.set_particles(4, np.array(sigma, F), 1.0)
        return e2
    returns = ev.particle_returns(obs[None], seq)
    assert returns.shape == (9, 4, 1) and ev(obs[None], seq).shape == (9, 1)
    np.testing.assert_array_equal(returns, fresh(fn.members).evaluate_particles(obs[None], seq)[1])
    assert not np.array_equal(returns, fresh(None).evaluate_particles(obs[None], seq)[1])
    det = DeterministicTrajectoryEvaluator(pendulum_reward_function, handler)
    plain = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=8)
    plain.set_mlp(fn.weights, fn.biases, fn.activation_codes, stats)
    np.testing.assert_array_equal(det(obs[None], seq), plain.evaluate(obs[None], seq))
    # a refit of one member alone reaches the engines (the function's version bumps)
    fn.members[1].set_weights(fn.members[0].weights, fn.members[0].biases)
    np.testing.assert_array_equal(ev.particle_returns(obs[None], seq), fresh(None).evaluate_particles(obs[None], seq)[1])
    with pytest.raises(ValueError):
        ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=3, process_noise_std=sigma)
