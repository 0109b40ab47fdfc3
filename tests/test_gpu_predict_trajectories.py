"""Open-loop trajectory prediction (bbmpc_predict_trajectories[_dev]) and the multi-step model error.

The oracle is oracle/oracle_np.py as it is: Evaluator.predict_next_state / evaluate_next_reward composed Hq times
(tests/traj_util.py).  Whole trajectories are held to the float64 yardstick described there: the device's deviation from
a float64 evaluation of the recurrence at most 4 x the float32 oracle's own, plus the one-step tolerance, no element
excused.  Start states were chosen on the CPU so that the oracle's deviation at the last step stays below 1e-3
(measured: <= 9.1e-7 for the learned models, <= 7.1e-5 for the pendulum at t = 50 / 30).  Every handle's planning
horizon differs from the Hq of the call."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import traj_util as T

pytestmark = pytest.mark.gpu
F = np.float32
CODE = {None: 0, "tanh": 1, "relu": 2, "sigmoid": 3, "swish": 10}


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _mlp_engine(L, c, horizon=7, agents=1, reward=None):
    from blackbox_mpc_amd.engine import Engine
    eng = Engine(L.OPT_NONE, L.DYN_MLP, reward or L.REW_PENDULUM, [-1.0] * c["U"], [1.0] * c["U"], dim_s=c["S"], num_agents=agents,
                 planning_horizon=horizon)
    eng.set_mlp(c["ws"], c["bs"], [CODE[a] for a in c["acts"]], c["stats"])
    return eng


def _pendulum_engine(L, strict, horizon=7, agents=1):
    from blackbox_mpc_amd.engine import Engine
    return Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=agents, planning_horizon=horizon,
                  quirks=L.STRICT_MATH if strict else 0)


PENDULUM_EV = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))


# ---- 1. step 0 is the one-step call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mlp200_norm_B4099_H50", "mlp64_S17U6_B77_H30", "mlp32_norm_B1_H50"])
def test_step0_is_the_one_step_call_mlp(L, name):
    c = T.mlp_case(name)
    got_s, got_r = _mlp_engine(L, c).predict_trajectories(c["states"], c["seq"])
    ev = T.oracle_mlp_evaluator(c)
    want = ev.predict_next_state(c["states"], c["seq"][:, 0])
    np.testing.assert_allclose(got_s[:, 0], want, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(got_r[:, 0], ev.evaluate_next_reward(c["states"], want, c["seq"][:, 0]), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("strict", [False, True])
def test_step0_is_the_one_step_call_pendulum(L, strict):
    c = T.pendulum_case("pendulum_B77_H50")
    got_s, got_r = _pendulum_engine(L, strict).predict_trajectories(c["states"], c["seq"])
    want = PENDULUM_EV.predict_next_state(c["states"], c["seq"][:, 0])
    np.testing.assert_allclose(got_s[:, 0], want, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(got_r[:, 0], PENDULUM_EV.evaluate_next_reward(c["states"], want, c["seq"][:, 0]), rtol=1e-4, atol=1e-3)


# ---- 2. whole trajectories against the oracle, bounded through float64 ---------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.MLP_CASES))
def test_mlp_trajectories_against_the_oracle(L, name):
    c = T.mlp_case(name)
    got_s, got_r = _mlp_engine(L, c).predict_trajectories(c["states"], c["seq"])
    assert got_s.shape == c["seq"].shape[:2] + (c["S"],) and got_r.shape == c["seq"].shape[:2]
    want_s, want_r = T.oracle_trajectories(T.oracle_mlp_evaluator(c), c["states"], c["seq"])
    s64, r64 = T.trajectories64(T.Mlp64(c["ws"], c["bs"], c["acts"], c["stats"]), c["states"], c["seq"])
    T.check_against_float64(got_s, want_s, s64, T.STATE_RTOL, T.STATE_ATOL, name + " states")
    T.check_against_float64(got_r, want_r, r64, T.REWARD_RTOL, T.REWARD_ATOL, name + " rewards")


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", sorted(T.PENDULUM_CASES))
def test_pendulum_trajectories_against_the_oracle(L, name, strict):
    c = T.pendulum_case(name)
    got_s, got_r = _pendulum_engine(L, strict).predict_trajectories(c["states"], c["seq"])
    want_s, want_r = T.oracle_trajectories(PENDULUM_EV, c["states"], c["seq"])
    s64, r64 = T.trajectories64(T.pendulum_step64, c["states"], c["seq"])
    what = "%s %s" % (name, "strict" if strict else "turn")
    T.check_against_float64(got_s, want_s, s64, T.STATE_RTOL, T.STATE_ATOL, what + " states")
    T.check_against_float64(got_r, want_r, r64, T.REWARD_RTOL, T.REWARD_ATOL, what + " rewards")


# ---- 3. consistency with the evaluator and the one-step call ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mlp", "pendulum", "pendulum_strict"])
def test_consistent_with_evaluate_and_predict_next_state(L, kind):
    N, A, H = 40, 3, 12
    rng = np.random.default_rng(3)
    if kind == "mlp":
        c = T.mlp_case("mlp200_norm_B4099_H50")
        eng = _mlp_engine(L, c, horizon=H, agents=A)
        states, lo = c["states"][:A], 1.0
    else:
        eng = _pendulum_engine(L, kind == "pendulum_strict", horizon=H, agents=A)
        states, lo = O.pendulum_start_states(A), 2.0
    seq = rng.uniform(-lo, lo, (N, A, H, eng.U)).astype(F)
    rows_s = np.tile(states, (N, 1))                                  # row b = n * A + a, as the evaluator flattens
    got_s, got_r = eng.predict_trajectories(rows_s, seq.reshape(N * A, H, eng.U))
    np.testing.assert_allclose(got_r.sum(1).reshape(N, A), eng.evaluate(states, seq), rtol=1e-3, atol=1e-3 * H)
    s = rows_s
    for t in range(H):
        s = eng.predict_next_state(s, seq.reshape(N * A, H, eng.U)[:, t])
    np.testing.assert_allclose(got_s[:, -1], s, rtol=2e-5, atol=2e-5 * H)


# ---- 4. user functions ---------------------------------------------------------------------------------------------------
def test_hip_source_functions_with_per_agent_parameters_and_t(L):
    from blackbox_mpc_amd.engine import Engine
    from tests.test_gpu_user_params import DYNAMICS_SIG, MASS_PENDULUM, TRACKING_REWARD
    A, per, Hq, S = 3, 5, 9, 3
    eng = Engine(L.OPT_NONE, L.DYN_USER, L.REW_USER, [-2.0], [2.0], dim_s=S, num_agents=A, planning_horizon=4)
    eng.set_dynamics_source(MASS_PENDULUM.replace("@SIG@", DYNAMICS_SIG[1]).replace("$0", "params[0]"), 1)
    eng.set_reward_source(TRACKING_REWARD, Hq * S)
    base = eng.compile_count()
    rng = np.random.default_rng(11)
    mass = np.array([[1.0], [1.5], [0.7]], F)
    ref = rng.uniform(-1, 1, (A, Hq, S)).astype(F)
    eng.set_user_params(L.USER_KIND_DYNAMICS, mass)
    eng.set_user_params(L.USER_KIND_REWARD, ref.reshape(A, -1))
    states = np.repeat(O.pendulum_start_states(A), per, axis=0)      # row b belongs to agent b / (B / A)
    seq = rng.uniform(-2, 2, (A * per, Hq, 1)).astype(F)
    got_s, got_r = eng.predict_trajectories(states, seq)
    assert eng.compile_count() == base + 1                           # bbmpc_user_traj, built on the first prediction
    # NumPy restatement (float32 oracle forms)
    s = states
    for t in range(Hq):
        th = O.atan2_32(s[:, 1], s[:, 0])
        m = np.repeat(mass[:, 0], per)
        acc = (F(-15.0) * O.sin32((th + O.PI32).astype(F))).astype(F)
        acc = (acc + ((F(3.0) / m).astype(F) * seq[:, t, 0]).astype(F)).astype(F)
        nthd = (s[:, 2] + (acc * F(0.05)).astype(F)).astype(F)
        nth = (th + (nthd * F(0.05)).astype(F)).astype(F)
        nthd = np.clip(nthd, F(-8), F(8))
        new = np.stack([O.cos32(nth), O.sin32(nth), nthd], 1)
        nxt = ((new - s).astype(F) + s).astype(F)
        d = nxt - np.repeat(ref[:, t], per, axis=0)
        np.testing.assert_allclose(got_s[:, t], nxt, rtol=2e-5, atol=2e-5)     # lock step: the one-step tolerance
        np.testing.assert_allclose(got_r[:, t], -(d * d).sum(1), rtol=1e-4, atol=1e-3)
        s = got_s[:, t]                                              # lock step: every step is checked from the device's state
    eng.set_user_params(L.USER_KIND_REWARD, (ref * F(0.5)).reshape(A, -1))
    again_s, _ = eng.predict_trajectories(states, seq)
    assert eng.compile_count() == base + 1                           # later calls and parameter updates compile nothing
    assert np.array_equal(again_s, got_s)                            # (the dynamics' parameters did not change)
    with pytest.raises(L.BBMPCError) as ex:                          # B % A != 0 with per-agent parameters
        eng.predict_trajectories(states[:A * per - 1], seq[:A * per - 1])
    assert ex.value.code == L.E_INVALID and "multiple of num_agents" in str(ex.value)


def test_a_handle_that_never_predicts_compiles_what_it_always_did(L):
    from blackbox_mpc_amd.engine import Engine
    from tests.test_gpu_user_functions import USER_PENDULUM_MODEL
    eng = Engine(L.OPT_NONE, L.DYN_USER, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=2, planning_horizon=5)
    eng.set_dynamics_source(USER_PENDULUM_MODEL)
    assert eng.compile_count() == 1                                  # the rows program
    seq = np.random.default_rng(0).uniform(-2, 2, (8, 2, 5, 1)).astype(F)
    eng.evaluate(O.pendulum_start_states(2), seq)
    assert eng.compile_count() == 2                                  # + the fused rollout, built on first use: the parent's count
    got, _ = eng.predict_trajectories(O.pendulum_start_states(4), seq[:4, 0])
    assert eng.compile_count() == 3                                  # + the trajectory kernel, on the first prediction only
    eng.predict_trajectories(O.pendulum_start_states(4), seq[:4, 0])
    assert eng.compile_count() == 3
    want, _ = _pendulum_engine(L, True).predict_trajectories(O.pendulum_start_states(4), seq[:4, 0])
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5 * 5)  # the user's pendulum against the built-in strict form


def _one_step_loop(ev, states, seq):
    s, out_s, out_r = states, [], []
    for t in range(seq.shape[1]):
        nxt = ev.predict_next_state(s, seq[:, t])
        out_r.append(ev.evaluate_next_reward(s, nxt, seq[:, t]))
        out_s.append(nxt)
        s = nxt
    return np.stack(out_s, 1), np.stack(out_r, 1)


def test_torch_callables_match_one_step_calls(L):
    import torch
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    S, U, B, Hq = 4, 2, 37, 6
    W = torch.tensor(np.random.default_rng(5).normal(0, 0.2, (S + U, S)).astype(F))

    def dyn(x, train=False):
        return torch.tanh(x @ W.to(x.device))

    def rew(cur, act, nxt):
        return -(nxt * nxt).sum(1) - 0.1 * (act * act).sum(1)

    h = SystemDynamicsHandler(Box(-np.ones(U, F), np.ones(U, F)), Box(-np.ones(S, F) * 10, np.ones(S, F) * 10),
                              dynamics_function=dyn, true_model=False, is_normalized=False)
    ev = DeterministicTrajectoryEvaluator(rew, h)
    rng = np.random.default_rng(6)
    states, seq = rng.normal(0, 0.5, (B, S)).astype(F), rng.uniform(-1, 1, (B, Hq, U)).astype(F)
    got_s, got_r = ev.predict_trajectories(states, seq)
    want_s, want_r = _one_step_loop(ev, states, seq)
    np.testing.assert_allclose(got_s, want_s, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(got_r, want_r, rtol=1e-4, atol=1e-3)


def test_mlp_with_inverse_transform_matches_one_step_calls(L):
    from blackbox_mpc_amd.engine import Engine
    from tests.test_gpu_user_params import IDENTITY_XFORM
    c = T.mlp_case("mlp200_norm_B4099_H50")
    eng = _mlp_engine(L, c)
    eng.set_inverse_transform_source(IDENTITY_XFORM)
    base = eng.compile_count()
    states, seq = c["states"][:45], c["seq"][:45, :8]
    got_s, got_r = eng.predict_trajectories(states, seq)
    assert eng.compile_count() == base
    s = states
    for t in range(seq.shape[1]):
        nxt = eng.predict_next_state(s, seq[:, t])
        np.testing.assert_allclose(got_s[:, t], nxt, rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(got_r[:, t], eng.evaluate_next_reward(s, nxt, seq[:, t]), rtol=1e-4, atol=1e-3)
        s = nxt


# ---- 5. outputs and errors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mlp", "pendulum"])
def test_outputs_errors_streams_and_repeatability(L, kind):
    import ctypes
    import torch
    if kind == "mlp":
        c = T.mlp_case("mlp200_raw_B77_H30")
        eng = _mlp_engine(L, c)
    else:
        c = T.pendulum_case("pendulum_B77_H50")
        eng = _pendulum_engine(L, False)
    states, seq = c["states"], c["seq"]
    B, Hq = seq.shape[:2]
    both_s, both_r = eng.predict_trajectories(states, seq)
    again_s, again_r = eng.predict_trajectories(states, seq)
    assert np.array_equal(both_s, again_s) and np.array_equal(both_r, again_r)
    only_s, none_r = eng.predict_trajectories(states, seq, want_rewards=False)
    none_s, only_r = eng.predict_trajectories(states, seq, want_states=False)
    assert none_r is None and none_s is None
    assert np.array_equal(only_s, both_s) and np.array_equal(only_r, both_r)
    for args, what in (((L.ptr(states), L.ptr(seq), B, Hq, None, None), "both null"),
                       ((L.ptr(states), L.ptr(seq), 0, Hq, L.ptr(both_s), None), "batch"),
                       ((L.ptr(states), L.ptr(seq), B, 0, L.ptr(both_s), None), "horizon"),
                       ((L.ptr(states), L.ptr(seq), B, 4097, L.ptr(both_s), None), "horizon")):
        assert L.lib.bbmpc_predict_trajectories(eng._h, *args) == L.E_INVALID
        assert what in L.lib.bbmpc_last_error().decode()
    # the device variant on a non-default stream: the same bits
    dev = torch.device("cuda", eng.device)
    side = torch.cuda.Stream(dev)
    d_s, d_q = torch.from_numpy(states).to(dev), torch.from_numpy(seq).to(dev)
    d_os, d_or = torch.empty((B, Hq, eng.S), device=dev), torch.empty((B, Hq), device=dev)
    torch.cuda.synchronize(dev)
    eng.set_torch_stream(side)
    eng.predict_trajectories_dev(d_s.data_ptr(), d_q.data_ptr(), B, Hq, d_os.data_ptr(), d_or.data_ptr())
    eng.synchronize()
    assert np.array_equal(d_os.cpu().numpy(), both_s) and np.array_equal(d_or.cpu().numpy(), both_r)
    eng.set_stream(0)


def test_weights_not_set_is_a_state_error(L):
    from blackbox_mpc_amd.engine import Engine
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_CHEETAH, [-1.0] * 6, [1.0] * 6, dim_s=20, num_agents=1, planning_horizon=3)
    with pytest.raises(L.BBMPCError) as ex:
        eng.predict_trajectories(np.zeros((4, 20), F), np.zeros((4, 5, 6), F))
    assert ex.value.code == L.E_STATE


def test_serves_a_handle_with_an_optimizer_and_a_resident_kernel(L):
    """any handle serves: a CEM pendulum handle whose control-step kernel is resident is stopped first"""
    from blackbox_mpc_amd.engine import Engine
    eng = Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=10,
                 population_size=128, max_iterations=2, num_elite=16, seed=1)
    st = O.pendulum_start_states(1)
    a0 = eng.optimize(st)
    c = T.pendulum_case("pendulum_B77_H50")
    got_s, _ = eng.predict_trajectories(c["states"], c["seq"])
    want_s, _ = _pendulum_engine(L, False).predict_trajectories(c["states"], c["seq"])
    assert np.array_equal(got_s, want_s)
    eng.optimize(st)


# ---- 7. multi-step error ---------------------------------------------------------------------------------------------------
def _episodes(step, rng, n_ep, T_, A, S, U, lo, start):
    obs_all, act_all = [], []
    for e in range(n_ep):
        steps = T_ - 3 * e                                           # episodes of different lengths
        acts = rng.uniform(-lo, lo, (steps, A, U)).astype(F)
        obs = np.zeros((steps + 1, A, S), F)
        obs[0] = start(A, e)
        for t in range(steps):
            obs[t + 1] = step(obs[t], acts[t])
        obs_all.append(obs)
        act_all.append(acts)
    return obs_all, act_all


def test_multistep_error_of_the_true_model_on_its_own_episodes(L):
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import multistep_windows
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel
    rng = np.random.default_rng(2)
    obs, acts = _episodes(lambda s, a: PENDULUM_EV.predict_next_state(s, a), rng, 3, 40, 2, 3, 1, 2.0,
                          lambda A, e: O.pendulum_start_states(A, agent_offset=10 * e))
    h = SystemDynamicsHandler(Box(np.array([-2.0], F), np.array([2.0], F)), Box(-np.ones(3, F) * 8, np.ones(3, F) * 8),
                              dynamics_function=PendulumTrueModel(), true_model=True)
    horizon = 30
    rmse, n = h.multistep_error(obs, acts, horizon, stride=2)
    starts, a_w, o_w = multistep_windows(obs, acts, horizon, 2)
    assert n == starts.shape[0] and rmse.shape == (horizon, 3)
    # the episodes ARE the float32 oracle's trajectories: the bound of check 2 with the oracle's own deviation from float64
    s64, _ = T.trajectories64(T.pendulum_step64, starts, a_w)
    dev_o = T.per_step_dev(o_w, s64)
    bound = T.FACTOR * dev_o + T.STATE_ATOL + T.STATE_RTOL * np.abs(s64).max()
    print("true-model rmse per step (max over s):", rmse.max(1), "bound:", bound)
    assert (rmse.max(1) <= bound).all()
    assert h.multistep_rmse[1] == n


def test_multistep_error_of_a_learned_model(L):
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import multistep_windows
    from blackbox_mpc_amd.spaces import Box
    c = T.mlp_case("mlp64_S17U6_B77_H30")
    S, U = c["S"], c["U"]
    m = DeterministicMLP([S + U, 64, 64, S], c["acts"])
    m.set_weights(c["ws"], c["bs"])
    h = SystemDynamicsHandler(Box(-np.ones(U, F), np.ones(U, F)), Box(-np.ones(S, F) * 10, np.ones(S, F) * 10), dynamics_function=m,
                              true_model=False, is_normalized=True)
    h.set_normalization_stats(*c["stats"])
    rng = np.random.default_rng(9)
    # "observed" episodes: a random walk (the model is wrong about them, so the error is far from zero)
    obs, acts = _episodes(lambda s, a: (s + 0.05 * rng.standard_normal(s.shape)).astype(F), rng, 4, 25, 3, S, U, 1.0,
                          lambda A, e: (rng.standard_normal((A, S)) * 0.3).astype(F))
    horizon, stride = 10, 3
    rmse, n = h.multistep_error(obs, acts, horizon, stride)
    brute = 0
    for o_, a_ in zip(obs, acts):                                    # window count and dropped windows, by brute force
        for agent in range(a_.shape[1]):
            for t0 in range(0, a_.shape[0], stride):
                if t0 + horizon <= a_.shape[0]:
                    brute += 1
    assert n == brute
    starts, a_w, o_w = multistep_windows(obs, acts, horizon, stride)
    pred, _ = _mlp_engine(L, c).predict_trajectories(starts, a_w)
    want = np.sqrt(((pred.astype(np.float64) - o_w.astype(np.float64)) ** 2).mean(0))
    np.testing.assert_allclose(rmse, want, rtol=1e-5)
    rmse2, _ = h.multistep_error(obs, acts, horizon, stride)
    assert np.array_equal(rmse, rmse2)
    rmse3, _ = h.multistep_error(obs, acts, horizon, stride, max_rows=50)      # chunked: the same sums in chunk order
    np.testing.assert_allclose(rmse3, rmse, rtol=1e-12)
    with pytest.raises(ValueError):
        h.multistep_error(obs, acts, 200)


def test_mlp_trajectories_with_the_cheetah_reward(L):
    """reward_generic's cheetah branch inside k_traj_mlp: the oracle's reward on the DEVICE's own states (lock step, so a
    threshold cannot fall differently) at the one-step reward tolerance"""
    c = T.mlp_case("mlp200_norm_B4099_H50")
    eng = _mlp_engine(L, c, reward=L.REW_CHEETAH)
    states, seq = c["states"][:333], c["seq"][:333, :20]
    got_s, got_r = eng.predict_trajectories(states, seq)
    cur = states
    for t in range(seq.shape[1]):
        np.testing.assert_allclose(got_r[:, t], O.cheetah_reward(cur, seq[:, t], got_s[:, t]), rtol=1e-4, atol=1e-3)
        cur = got_s[:, t]
    assert np.abs(got_r).max() > 1.0                                 # (the thresholds and the velocity term are exercised)


# ---- 6. plan readback -----------------------------------------------------------------------------------------------------
OPTIMIZERS = {"CEM": dict(population_size=64, num_elite=8, max_iterations=3), "PI2": dict(population_size=64, max_iterations=3),
              "RandomSearch": dict(population_size=64), "PSO": dict(population_size=64, max_iterations=3),
              "SPSA": dict(population_size=64, max_iterations=3), "CMA-ES": dict(population_size=64, num_elite=8, max_iterations=3)}
PLAN_A, PLAN_H = 2, 8


def _plan_policy(model, name, seed=3):
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    if model == "pendulum":
        from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
        act, obs = Box(np.array([-2.0], F), np.array([2.0], F)), Box(-np.ones(3, F) * 8, np.ones(3, F) * 8)
        h = SystemDynamicsHandler(act, obs, dynamics_function=PendulumTrueModel(), true_model=True)
        rew, start = pendulum_reward_function, O.pendulum_start_states(PLAN_A)
    else:
        from blackbox_mpc_amd.utils.cheetah import reward_function as rew
        c = T.mlp_case("mlp200_norm_B4099_H50")
        m = DeterministicMLP([26, 200, 200, 20], c["acts"])
        m.set_weights(c["ws"], c["bs"])
        act, obs = Box(-np.ones(6, F), np.ones(6, F)), Box(-np.ones(20, F) * 10, np.ones(20, F) * 10)
        h = SystemDynamicsHandler(act, obs, dynamics_function=m, true_model=False, is_normalized=True)
        h.set_normalization_stats(*c["stats"])
        start = c["states"][:PLAN_A]
    pol = MPCPolicy(reward_function=rew, env_action_space=act, env_observation_space=obs, dynamics_handler=h, optimizer_name=name,
                    num_agents=PLAN_A, planning_horizon=PLAN_H, seed=seed, **OPTIMIZERS[name])
    return pol, start


def _inject(L, eng, name, rng):
    """standard draws in the reference layout for the optimizers whose draws are one tensor per iteration; PSO (five kinds
    of draws) runs on the engine's own seeded generator, which the traced twin reproduces"""
    N, A, H, U, it = eng.N, eng.A, eng.H, eng.U, max(eng.iters, 1)
    if name in ("CEM", "PI2"):
        eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack([O.truncated_normal_noise(rng, (N, A, H, U)) for _ in range(it)]))
    elif name == "RandomSearch":
        eng.inject_noise(L.NOISE_UNIFORM, rng.uniform(0, 1, (N, A, H, U)).astype(F))
    elif name == "SPSA":
        eng.inject_noise(L.NOISE_RADEMACHER, rng.choice([-1.0, 1.0], (it, N, A, H, U)).astype(F))
    elif name == "CMA-ES":
        eng.inject_noise(L.NOISE_NORMAL, rng.standard_normal((it, N, A * H * U)).astype(F))


@pytest.mark.parametrize("model", ["pendulum", "mlp"])
@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_plan_is_the_solution_the_action_came_from(L, name, model):
    pol, start = _plan_policy(model, name)
    eng = pol._optimizer._engine
    _inject(L, eng, name, np.random.default_rng(17))
    pol.act(start, 0)                                                # a call with the switch off ...
    with pytest.raises(RuntimeError, match="keep_plan"):
        pol.plan(start)                                              # ... leaves nothing to read, and says how to switch it on
    pol.keep_plan(True)
    with pytest.raises(RuntimeError, match="keep_plan"):
        pol.plan(start)                                              # the switch has to be on DURING the call
    action, nxt, rew = pol.act(start, 1)
    p_act, p_states, p_rew = pol.plan(start)
    assert p_act.shape == (PLAN_A, PLAN_H, eng.U) and p_states.shape == (PLAN_A, PLAN_H, eng.S) and p_rew.shape == (PLAN_A, PLAN_H)
    assert np.array_equal(p_act[:, 0], action)                       # exactly: no exploration noise
    np.testing.assert_allclose(p_states[:, 0], nxt, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(p_rew[:, 0], rew, rtol=1e-4, atol=1e-3)
    # a traced twin: same seed, same draws, same two calls
    twin, _ = _plan_policy(model, name)
    te = twin._optimizer._engine
    _inject(L, te, name, np.random.default_rng(17))
    te.set_trace(True)
    twin.act(start, 0)
    t_action, _, _ = twin.act(start, 1)
    assert np.array_equal(t_action, action)
    if name == "RandomSearch":
        best, samples = te.get_trace(0, L.TRACE_ELITES), te.get_trace(0, L.TRACE_SAMPLES)
        want = np.stack([samples[best[a], a] for a in range(PLAN_A)])
    else:
        want = te.get_trace(te.iters - 1, L.TRACE_MEAN)              # (PSO: the global best is recorded there)
    assert np.array_equal(p_act, want)
    one = pol.plan(start[0])                                         # 1-D un-batching, as act
    assert one[0].shape == (PLAN_H, eng.U) and np.array_equal(one[1], p_states[0])


@pytest.mark.parametrize("model,name", [("pendulum", "CEM"), ("mlp", "PI2")])
def test_with_the_plan_switch_off_nothing_changes(L, model, name):
    """a handle whose switch went on and off again before any call computes, and is served, exactly as one that never saw it"""
    a, start = _plan_policy(model, name)
    b, _ = _plan_policy(model, name)
    b.keep_plan(True)
    b.keep_plan(False)
    for t in range(8):
        ra, rb = a.act(start, t), b.act(start, t)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y)
    ea, eb = a._optimizer._engine, b._optimizer._engine
    assert ea.call_stats() == eb.call_stats() and ea.graph_stats() == eb.graph_stats()
    if model == "mlp":
        assert eb.graph_stats() > 0                                  # the steady-state step is still replayed as a graph
    with pytest.raises(RuntimeError, match="keep_plan"):
        b.plan(start)
