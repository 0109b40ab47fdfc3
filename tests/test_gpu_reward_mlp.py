"""GPU tests of learned reward models (BBMPC_REW_MLP, csrc/kernels_reward_mlp.hpp) through the C ABI.

Against the statement (tests/reward_mlp_util.py, float64): the states come from predict_trajectories, whose state path is the
learned model's existing code; per-step rewards and evaluate_next_reward are held to tests/test_gpu_mlp.py's one-step
tolerance (rtol 2e-5 + atol 2e-5, network outputs O(1)), evaluate to its H-step tolerance (rtol 1e-3 + atol 1e-3 H).
Against the existing HIP-source path: a twin handle takes the same network as a HipRewardFunction with its weights as
runtime parameters; all six optimizers run on both in lock step (same injected draws) under tests/bounds_util.NARROW, an
asymmetric bound set that clips on both sides.  That candidates were clipped is asserted for every optimizer that clips:
from the handle's own sample trace where it holds the feasible candidates (PI2, CMA-ES: elements exactly at a bound), and
for SPSA and PSO, whose candidates inside an iteration are not traced, from tests/bounds_util's recording oracle run on the
same network, bounds, start state and draws (the unclipped argument of every clip, as tests/test_gpu_optimizer_bounds.py
uses it).  RandomSearch and CEM draw inside the bounds and never clip."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import bounds_util as B
from tests import reward_mlp_util as R

pytestmark = pytest.mark.gpu
F = np.float32
DYN_ACT = {"tanh": 1, None: 0}


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _dynamics(S, U, hidden, seed=42):
    dims = [S + U] + hidden + [S]
    ws, bs = O.make_mlp_params(dims, seed=seed)
    rng = np.random.default_rng(seed + 2)
    stats = [rng.normal(0, 0.2, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F), rng.normal(0, 0.1, U).astype(F),
             rng.uniform(0.5, 1.5, U).astype(F), rng.normal(0, 0.01, S).astype(F), rng.uniform(0.05, 0.15, S).astype(F)]
    return ws, bs, [DYN_ACT["tanh"]] * len(hidden) + [DYN_ACT[None]], stats


def _engine(L, net, A=1, H=1, opt=None, lo=None, hi=None, twin=False, hidden=None, **kw):
    from blackbox_mpc_amd.engine import Engine
    lo = [-1.0] * net.U if lo is None else lo
    hi = [1.0] * net.U if hi is None else hi
    eng = Engine(L.OPT_NONE if opt is None else opt, L.DYN_MLP, L.REW_USER if twin else L.REW_MLP, lo, hi, dim_s=net.S,
                 num_agents=A, planning_horizon=H, **kw)
    eng.set_mlp(*_dynamics(net.S, net.U, hidden or [24]))
    if twin:
        src, params = R.twin_source_and_params(net)
        eng.set_reward_source(src, params.size)
        eng.set_user_params(L.USER_KIND_REWARD, params)
    else:
        eng.set_reward_mlp(net.ws, net.bs, net.codes(), net.mask, net.stats)
    return eng


def _states(net, A, seed=5):
    return np.random.default_rng(seed).normal(0, 0.5, (A, net.S)).astype(F)


def _check_against_statement(L, net, N, A, H, hidden=None):
    eng = _engine(L, net, A=A, H=H, hidden=hidden)
    rng = np.random.default_rng(N + H)
    state = _states(net, A)
    seq = rng.uniform(-1, 1, (N, A, H, net.U)).astype(F)
    rows_s = np.broadcast_to(state[None], (N, A, net.S)).reshape(N * A, net.S)
    rows_q = seq.reshape(N * A, H, net.U)
    states_out, rewards_out = eng.predict_trajectories(rows_s, rows_q)
    want = R.per_step(net, rows_s, states_out, rows_q)
    assert np.all(np.isfinite(want)) and 0.2 < np.std(want) < 20
    rt, at = R.ONE_STEP
    np.testing.assert_allclose(rewards_out, want, rtol=rt, atol=at)
    cur = np.concatenate([rows_s[:, None], states_out[:, :-1]], 1).reshape(N * A * H, net.S)
    got1 = eng.evaluate_next_reward(cur, states_out.reshape(N * A * H, net.S), rows_q.reshape(N * A * H, net.U))
    np.testing.assert_allclose(got1, want.reshape(-1), rtol=rt, atol=at)
    got = eng.evaluate(state, seq)
    np.testing.assert_allclose(got, R.returns(want).reshape(N, A), rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    np.testing.assert_array_equal(eng.evaluate(state, seq), got)           # two identical calls: identical bits
    return eng


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("net", R.small_nets(), ids=lambda n: n.name)
def test_small_networks_against_the_statement(L, net, H):
    _check_against_statement(L, net, 37, 2, H)


def test_medium_network_against_the_statement(L):
    _check_against_statement(L, R.medium_net(), 50, 2, 4, hidden=[200, 200])


def test_network_at_the_limits_fits_the_lds(L):
    _check_against_statement(L, R.limits_net(), 16, 2, 2)


# ---- against the HIP-source twin --------------------------------------------------------------------------------------
def _twin_nets():
    return [n for n in R.small_nets() if n.n_params() <= 4096]


@pytest.mark.parametrize("net", _twin_nets(), ids=lambda n: n.name)
def test_twin_evaluate_predict_and_one_step(L, net):
    N, A, H = 37, 2, 5
    a, b = _engine(L, net, A=A, H=H), _engine(L, net, A=A, H=H, twin=True)
    rng = np.random.default_rng(1)
    state, seq = _states(net, A), rng.uniform(-1, 1, (N, A, H, net.U)).astype(F)
    np.testing.assert_allclose(a.evaluate(state, seq), b.evaluate(state, seq), rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    rows_s, rows_q = rng.normal(0, 0.5, (N, net.S)).astype(F), rng.uniform(-1, 1, (N, 7, net.U)).astype(F)
    (sa, ra), (sb, rb) = a.predict_trajectories(rows_s, rows_q), b.predict_trajectories(rows_s, rows_q)
    rt, at = R.ONE_STEP
    np.testing.assert_allclose(sa, sb, rtol=rt, atol=at)
    np.testing.assert_allclose(ra, rb, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * 7)    # (rewards behind up to seven model steps of two kernels)
    nxt = rng.normal(0, 0.5, (N, net.S)).astype(F)
    np.testing.assert_allclose(a.evaluate_next_reward(rows_s, nxt, rows_q[:, 0]), b.evaluate_next_reward(rows_s, nxt, rows_q[:, 0]),
                               rtol=rt, atol=at)


OPTS = ("RS", "CEM", "PI2", "SPSA", "PSO", "CMA")


def _opt(L, name):
    return {"RS": L.OPT_RANDOM_SEARCH, "CEM": L.OPT_CEM, "PI2": L.OPT_PI2, "SPSA": L.OPT_SPSA, "PSO": L.OPT_PSO, "CMA": L.OPT_CMAES}[name]


def _inject(L, eng, name, noise):
    if name == "RS":
        eng.inject_noise(L.NOISE_UNIFORM, noise["uniform"])
    elif name in ("CEM", "PI2"):
        eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    elif name == "SPSA":
        eng.inject_noise(L.NOISE_RADEMACHER, np.stack(noise["rademacher"]))
    elif name == "PSO":
        eng.inject_noise(L.NOISE_PSO_SCALARS, noise["normal2"])
        eng.inject_noise(L.NOISE_PSO_RESEED_TRUNC, noise["trunc"])
        eng.inject_noise(L.NOISE_PSO_RESEED_UNIFORM, noise["uniform"])
    else:
        eng.inject_noise(L.NOISE_NORMAL, np.stack(noise["normal"]))


@pytest.mark.parametrize("opt_name", OPTS)
def test_twin_control_steps_of_all_optimizers_under_clipping_bounds(L, opt_name):
    net = R.small_nets()[1]                                    # 7-20-1, inputs (s_t, a_t, s_{t+1}), normalised
    N, A, H, iters, k = 24, 2, 4, 2, 6
    lo, hi = B.NARROW
    noise = B.make_noise(opt_name, np.random.default_rng(B.case_seed("reward-mlp", opt_name)), A, net.U, n=N, h=H, iters=iters)
    state = _states(net, A)
    out = []
    for twin in (False, True):
        eng = _engine(L, net, A=A, H=H, opt=_opt(L, opt_name), lo=lo, hi=hi, twin=twin, population_size=N, max_iterations=iters,
                      num_elite=k, seed=3)
        eng.set_trace(True)
        if opt_name in ("CEM", "PI2"):                         # unit variance on a range of 0.5: the draws leave the bounds on both sides
            eng.set_state("var0", np.ones((A, H, net.U), F))
        _inject(L, eng, opt_name, noise)
        act, nxt, rew = eng.optimize(state)
        n_it = 1 if opt_name == "RS" else iters
        out.append((act, nxt, rew, [eng.get_trace(it, L.TRACE_REWARDS) for it in range(n_it)], eng))
    (act, nxt, rew, tr, eng), (act_t, nxt_t, rew_t, tr_t, _) = out
    for it, (r, r_t) in enumerate(zip(tr, tr_t)):
        np.testing.assert_allclose(r, r_t, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H, err_msg="iteration %d" % it)
    np.testing.assert_allclose(act, act_t, rtol=0, atol=2e-3)                  # test_gpu_mlp.py's lock-step action tolerance
    np.testing.assert_allclose(nxt, nxt_t, rtol=2e-5, atol=2e-3)
    np.testing.assert_allclose(rew, rew_t, rtol=1e-3, atol=1e-2)               # the record's reward, at actions 2e-3 apart
    lo_f, hi_f = F(lo[0]), F(hi[0])
    if opt_name in ("PI2", "CMA"):                            # the traced samples are the feasible candidates that were rolled out
        x = np.stack([eng.get_trace(it, L.TRACE_SAMPLES) for it in range(iters)])
        assert np.all((x >= lo_f) & (x <= hi_f))
        assert np.any(x == lo_f) and np.any(x == hi_f), (int((x == lo_f).sum()), int((x == hi_f).sum()))
    if opt_name in ("SPSA", "PSO"):
        ws, bs, _, stats = _dynamics(net.S, net.U, [24])
        ev = O.Evaluator(lambda c, a_, n: net.rows(c, a_, n).astype(F), O.Handler(O.MLP(ws, bs, ["tanh", None]), False, True, stats))
        run = B.Runner(opt_name, ev, lo, hi, A, n=N, h=H, iters=iters, k=k)
        act_o = run.step(state, noise)
        cov = B.clip_coverage(run.clips[0], lo, hi)
        assert cov["penalised"].sum() > 0 and (cov["at_lo"].sum() > 0 or cov["at_hi"].sum() > 0), cov
        if opt_name == "SPSA":                                 # (PSO's action is quirk Q4's all-zero personal best on both sides)
            np.testing.assert_allclose(act, act_o, rtol=0, atol=2e-3)


def test_several_steps_per_workgroup_and_a_ragged_last_chunk(L):
    """The scorer's in-workgroup loop over planning steps: with ceil(512 / tiles) < H a workgroup scores tchunk > 1 steps one
    after the other (LDS tiles rewritten per step) and, where H % tchunk != 0, the last chunk is short.  N = 2100, H = 5:
    132 tiles, 4 chunks, tchunk = 2, chunks of 2 + 2 + 1 steps.  N = 300, H = 29: 19 tiles, 27 chunks asked, tchunk = 2, 15
    chunks, the last of one step.  Against the statement, with the two-runs-equal-bits and the agent-split checks."""
    for net, N, H in ((R.small_nets()[1], 2100, 5), (R.small_nets()[4], 300, 29)):
        tiles = (N + 15) // 16
        chunks = max(1, min(H, (512 + tiles - 1) // tiles))
        tchunk = (H + chunks - 1) // chunks
        assert tchunk > 1 and H % tchunk != 0, (N, H, tchunk)
        A = 2
        eng = _engine(L, net, A=A, H=H)
        rng = np.random.default_rng(N)
        state = _states(net, A)
        seq = rng.uniform(-1, 1, (N, A, H, net.U)).astype(F)
        rows_s = np.broadcast_to(state[None], (N, A, net.S)).reshape(N * A, net.S)
        rows_q = seq.reshape(N * A, H, net.U)
        states_out, _ = eng.predict_trajectories(rows_s, rows_q, want_rewards=False)
        want = R.returns(R.per_step(net, rows_s, states_out, rows_q)).reshape(N, A)
        got = eng.evaluate(state, seq)
        np.testing.assert_allclose(got, want, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
        np.testing.assert_array_equal(eng.evaluate(state, seq), got)
        one = _engine(L, net, A=1, H=H, agent_offset=1, num_agents_global=A)
        np.testing.assert_array_equal(one.evaluate(state[1:2], np.ascontiguousarray(seq[:, 1:2])), got[:, 1:2])


# ---- refusals, error codes, handle behaviour -----------------------------------------------------------------------------
def _raises(L, code, fn):
    with pytest.raises(L.BBMPCError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


def test_refusals_and_error_codes(L):
    from blackbox_mpc_amd.engine import Engine
    net = R.small_nets()[1]
    N, A, H = 8, 1, 3
    state, seq = _states(net, A), np.zeros((N, A, H, net.U), F)
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_MLP, [-1.0], [1.0], dim_s=net.S, num_agents=A, planning_horizon=H)
    eng.set_mlp(*_dynamics(net.S, net.U, [24]))
    assert "bbmpc_set_reward_mlp" in _raises(L, L.E_STATE, lambda: eng.evaluate(state, seq))                 # compute before set
    assert "bbmpc_set_reward_mlp" in _raises(L, L.E_STATE, lambda: eng.evaluate_next_reward(state, state, np.zeros((A, 1), F)))
    good = (net.ws, net.bs, net.codes(), net.mask, net.stats)
    _raises(L, L.E_INVALID, lambda: eng.set_reward_mlp(net.ws[:1] + [np.zeros((20, 2), F)], net.bs[:1] + [np.zeros(2, F)], net.codes(), 7, None))
    _raises(L, L.E_INVALID, lambda: eng.set_reward_mlp(net.ws, net.bs, net.codes(), 3, None))                # D = 7 but the mask selects 4
    _raises(L, L.E_INVALID, lambda: eng.set_reward_mlp(net.ws, net.bs, net.codes(), 0, None))
    _raises(L, L.E_INVALID, lambda: eng.set_reward_mlp(net.ws, net.bs, [1, 99], 7, None))
    wide = [np.zeros((7, 513), F), np.zeros((513, 1), F)]
    _raises(L, L.E_UNSUPPORTED, lambda: eng.set_reward_mlp(wide, [np.zeros(513, F), np.zeros(1, F)], [1, 0], 7, None))
    deep = [np.zeros((7, 8), F)] + [np.zeros((8, 8), F)] * 7 + [np.zeros((8, 1), F)]
    _raises(L, L.E_UNSUPPORTED, lambda: eng.set_reward_mlp(deep, [np.zeros(w.shape[1], F) for w in deep], [1] * 9, 7, None))
    _raises(L, L.E_STATE, lambda: eng.evaluate(state, seq))                                                  # ... and nothing was installed
    eng.set_reward_mlp(*good)
    want = eng.evaluate(state, seq)
    assert "particles" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_particles(4, np.zeros(net.S, F), 0.0))
    assert "transform" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_inverse_transform_source(B.XFORM_SOURCE))
    _raises(L, L.E_INVALID, lambda: eng.set_reward_mlp(net.ws, net.bs, net.codes(), 3, None))
    np.testing.assert_array_equal(eng.evaluate(state, seq), want)                                            # the handle stays usable
    for dyn in (L.DYN_PENDULUM, L.DYN_USER):
        msg = _raises(L, L.E_UNSUPPORTED, lambda: Engine(L.OPT_NONE, dyn, L.REW_MLP, [-1.0], [1.0], dim_s=3, num_agents=1, planning_horizon=H))
        assert "BBMPC_DYN_MLP" in msg
    other = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-1.0], [1.0], dim_s=3, num_agents=1, planning_horizon=H)
    _raises(L, L.E_STATE, lambda: other.set_reward_mlp(*good))


def test_nan_weights_new_weights_agent_split(L):
    net = R.small_nets()[1]
    N, H = 37, 5
    rng = np.random.default_rng(2)
    state4, seq4 = _states(net, 4), rng.uniform(-1, 1, (N, 4, H, net.U)).astype(F)
    eng = _engine(L, net, A=4, H=H)
    full = eng.evaluate(state4, seq4)
    for off in (0, 2):                                         # a 2 + 2 agent split: bit for bit the A = 4 result
        half = _engine(L, net, A=2, H=H, agent_offset=off, num_agents_global=4)
        np.testing.assert_array_equal(half.evaluate(state4[off:off + 2], np.ascontiguousarray(seq4[:, off:off + 2])), full[:, off:off + 2])
    other = R.small_nets()[2]                                  # same shape, other weights, no statistics: replaced in place
    eng.set_reward_mlp(other.ws, other.bs, other.codes(), other.mask, other.stats)
    got = eng.evaluate(state4, seq4)
    assert np.max(np.abs(got - full)) > 0.1
    np.testing.assert_allclose(got, _engine(L, other, A=4, H=H).evaluate(state4, seq4), rtol=0, atol=0)
    bad = [w.copy() for w in net.ws]
    bad[0][0, 0] = np.nan
    eng.set_reward_mlp(bad, net.bs, net.codes(), net.mask, net.stats)
    np.testing.assert_array_equal(eng.evaluate(state4, seq4), np.full((N, 4), F(-1.0e6)))


# ---- the Python layer: learning utilities, evaluator, MPCPolicy, staleness ---------------------------------------------------
def test_python_layer_learns_plans_and_reuploads_a_refitted_model(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.policies import RandomPolicy
    from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.trajectory_evaluators.particle import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.dynamics_learning import learn_dynamics_from_policy
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    from blackbox_mpc_amd.utils.rollouts import ModelEnvironment, rollout_on_device
    act_space, obs_space = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    A, T = 3, 20
    start = O.pendulum_start_states(A)
    true_handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=PendulumTrueModel(), true_model=True)
    env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)
    model = LearnedRewardMLP(3, 1, [20, 1], ["tanh", None], inputs="sas", seed=1)
    v0 = model._version
    handler = learn_dynamics_from_policy(
        env, RandomPolicy(A, act_space, seed=0), number_of_rollouts=2, task_horizon=T,
        dynamics_function=DeterministicMLP(layers=[4, 16, 3], activation_functions=["tanh", None], seed=0), epochs=2, batch_size=32, seed=0,
        reward_model=model, reward_train_args=dict(epochs=2, batch_size=32, seed=0))
    assert model._version > v0 and model.normalization_stats() is not None and model._data[0].shape == (2 * T * A, 3)
    # the evaluator: H-step returns against the model's own NumPy statement on the engine's states, before and after new weights
    ev = DeterministicTrajectoryEvaluator(model, handler)
    rng = np.random.default_rng(0)
    N, H = 20, 4
    seq = rng.uniform(-2, 2, (N, A, H, 1)).astype(F)

    def statement():
        rows_s = np.broadcast_to(start[None], (N, A, 3)).reshape(N * A, 3)
        states, rewards = ev.predict_trajectories(rows_s, seq.reshape(N * A, H, 1))
        cur = np.concatenate([rows_s[:, None], states[:, :-1]], 1)
        want = model(cur.reshape(-1, 3), seq.reshape(-1, 1), states.reshape(-1, 3)).reshape(N * A, H)
        np.testing.assert_allclose(rewards, want, rtol=2e-5, atol=2e-5)
        return want.astype(np.float64).sum(1).reshape(N, A)
    first = ev(start, seq)
    np.testing.assert_allclose(first, statement(), rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    policy = MPCPolicy(reward_function=model, env_action_space=act_space, env_observation_space=obs_space, dynamics_handler=handler,
                       optimizer_name="CEM", num_agents=A, planning_horizon=H, population_size=64, num_elite=8, max_iterations=2)
    a1, n1, r1 = policy.act(start, 0)
    np.testing.assert_allclose(r1, model(start, a1, n1), rtol=2e-5, atol=2e-5)
    model.set_weights([w * F(-1.5) for w in model.weights], [b + F(0.25) for b in model.biases])            # "refitted"
    second = ev(start, seq)
    assert np.max(np.abs(second - first)) > 0.1
    np.testing.assert_allclose(second, statement(), rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    a2, n2, r2 = policy.act(start, 1)                          # the optimizer's engine uploads the new weights before it plans
    np.testing.assert_allclose(r2, model(start, a2, n2), rtol=2e-5, atol=2e-5)
    assert np.max(np.abs(r2 - r1)) > 1e-3
    # plan readback and the on-device episode go through the same handle
    policy.keep_plan(True)
    a3, _, _ = policy.act(start, 2)
    pa, ps, pr = policy.plan(start)
    np.testing.assert_array_equal(pa[:, 0], a3)
    cur = np.concatenate([start[:, None], ps[:, :-1]], 1)
    np.testing.assert_allclose(pr, model(cur.reshape(-1, 3), pa.reshape(-1, 1), ps.reshape(-1, 3)).reshape(A, H), rtol=2e-5, atol=2e-5)
    policy.keep_plan(False)
    acts, obs, rews = rollout_on_device(policy, start, 3)
    np.testing.assert_allclose(rews, model(obs[:-1].reshape(-1, 3), acts.reshape(-1, 1), obs[1:].reshape(-1, 3)).reshape(3, A),
                               rtol=2e-5, atol=2e-5)
    with pytest.raises(NotImplementedError, match="LearnedRewardMLP"):
        ParticleTrajectoryEvaluator(model, handler, 4, 0.01)
    with pytest.raises(NotImplementedError, match="learned model"):
        DeterministicTrajectoryEvaluator(model, true_handler)(start, seq)
