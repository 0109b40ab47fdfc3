"""GPU tests of learned terminal values (bbmpc_set_terminal_value_mlp, k_value_mlp_terminal) through the C ABI.

Against the statement (tests/terminal_value_util.py, float64): V on rows at tests/reward_mlp_util's one-step tolerance (rtol
2e-5 + atol 2e-5, outputs O(1)); evaluate with a network = evaluate on the same handle before it was set + w * V(s_H), s_H
from the handle's own predict_trajectories, at the H-step tolerance (rtol 1e-3 + atol 1e-3 H: the terminal state is compared
across two kernels).  Against the existing HIP-source path: a twin reward that evaluates the reward network at every step
and adds w * V(nxt) at the last one, all six optimizers in lock step under clipping bounds."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import bounds_util as B
from tests import particle_user_reward_util as RU
from tests import reward_mlp_util as R
from tests import terminal_value_util as V

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = ("builtin", "user", "mlp")


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
    return ws, bs, [1] * len(hidden) + [0], stats


REWARD_NET = R.small_nets()[1]                                 # 7-20-1, inputs (s_t, a_t, s_{t+1}), normalised


def _engine(L, kind, A=1, H=1, opt=None, lo=(-1.0,), hi=(1.0,), S=3, U=1, **kw):
    """DYN_MLP + {built-in pendulum, HIP-source MIXED_REWARD, learned reward} handle, S = 3, U = 1 unless said otherwise"""
    from blackbox_mpc_amd.engine import Engine
    rew = {"builtin": L.REW_PENDULUM, "user": L.REW_USER, "mlp": L.REW_MLP}[kind]
    eng = Engine(L.OPT_NONE if opt is None else opt, L.DYN_MLP, rew, list(lo), list(hi), dim_s=S, num_agents=A, planning_horizon=H, **kw)
    eng.set_mlp(*_dynamics(S, U, [24]))
    if kind == "user":
        eng.set_reward_source(RU.MIXED_REWARD)
    elif kind == "mlp":
        eng.set_reward_mlp(REWARD_NET.ws, REWARD_NET.bs, REWARD_NET.codes(), REWARD_NET.mask, REWARD_NET.stats)
    return eng


def _set(eng, net, w=1.0):
    eng.set_terminal_value_mlp(net.ws, net.bs, net.codes(), net.stats, w)


def _states(A, S=3, seed=5):
    return np.random.default_rng(seed).normal(0, 0.5, (A, S)).astype(F)


def _last_states(eng, state, seq):
    N, A, H, U = seq.shape
    rows_s = np.broadcast_to(state[None], (N, A, state.shape[1])).reshape(N * A, -1)
    states_out, _ = eng.predict_trajectories(rows_s, seq.reshape(N * A, H, U), want_rewards=False)
    return states_out[:, -1].reshape(N, A, -1)


def _raises(L, code, fn):
    with pytest.raises(L.BBMPCError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


# ---- 1. rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", V.small_nets() + [V.medium_net(), V.limits_net()], ids=lambda n: n.name)
def test_rows_against_the_statement(L, net):
    from blackbox_mpc_amd.engine import Engine
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM if net.S == 3 else L.REW_USER,
                 [-1.0], [1.0], dim_s=net.S, num_agents=1, planning_horizon=1)
    assert "bbmpc_set_terminal_value_mlp" in _raises(L, L.E_STATE, lambda: eng.evaluate_terminal_value(np.zeros((1, net.S), F)))
    _set(eng, net, 3.0)                                        # (the weight plays no part in the rows call)
    rt, at = R.ONE_STEP
    rng = np.random.default_rng(net.S)
    for b in (1, 16, 17, 37):
        s = rng.normal(0, 0.7, (b, net.S)).astype(F)
        want = V.value(net, s)
        got = eng.evaluate_terminal_value(s)
        print(net.name, b, "max |V - statement| = %.3g" % np.max(np.abs(got - want)))
        np.testing.assert_allclose(got, want, rtol=rt, atol=at)
    assert 0.2 < np.std(want) < 20


# ---- 2. evaluate, every reward kind ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1.0, -0.5])
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_adds_the_terminal_term_for_every_reward_kind(L, kind, H, w):
    N, A = 37, 2
    net = V.small_nets()[1]
    eng = _engine(L, kind, A=A, H=H)
    rng = np.random.default_rng(N + H)
    state, seq = _states(A), rng.uniform(-1, 1, (N, A, H, 1)).astype(F)
    before = eng.evaluate(state, seq)
    s_last = _last_states(eng, state, seq)
    _set(eng, net, w)
    got = eng.evaluate(state, seq)
    want = V.with_terminal(before, net, w, s_last)
    assert np.std(want - before) > 0.1                         # the term is not lost in the tolerance
    print(kind, H, w, "max |R' - statement| = %.3g" % np.max(np.abs(got - want)))
    np.testing.assert_allclose(got, want, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    np.testing.assert_array_equal(eng.evaluate(state, seq), got)
    # the one-step calls do not read the network
    nxt = eng.predict_next_state(state, seq[0, :, 0])
    eng.set_terminal_value_mlp(None, None, None)               # n_layers = 0
    np.testing.assert_array_equal(eng.predict_next_state(state, seq[0, :, 0]), nxt)
    after = eng.evaluate(state, seq)
    if kind in ("user", "mlp"):                                # the route did not change: bit for bit what it was
        np.testing.assert_array_equal(after, before)
    else:
        np.testing.assert_allclose(after, before, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)


# ---- 3. device against device: the HIP-source twin ---------------------------------------------------------------------------
def _pair(L, H, w, **kw):
    vnet = V.small_nets()[1]
    a = _engine(L, "mlp", H=H, **kw)
    _set(a, vnet, w)
    b = _engine(L, "user", H=H, **kw)
    src, params = V.twin_source_and_params(REWARD_NET, vnet, w, H)
    b.set_reward_source(src, params.size)
    b.set_user_params(L.USER_KIND_REWARD, params)
    return a, b


def test_twin_evaluate(L):
    N, A, H, w = 37, 2, 5, -0.5
    a, b = _pair(L, H, w, A=A)
    rng = np.random.default_rng(1)
    state, seq = _states(A), rng.uniform(-1, 1, (N, A, H, 1)).astype(F)
    ra, rb = a.evaluate(state, seq), b.evaluate(state, seq)
    print("twin evaluate: max diff %.3g" % np.max(np.abs(ra - rb)))
    np.testing.assert_allclose(ra, rb, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)


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
    N, A, H, iters, k, w = 24, 2, 4, 2, 6, 1.0                 # 24 candidates: a tile and a half
    lo, hi = B.NARROW
    a, b = _pair(L, H, w, A=A, opt=_opt(L, opt_name), lo=lo, hi=hi, population_size=N, max_iterations=iters, num_elite=k, seed=3)
    n_it = 1 if opt_name == "RS" else iters
    state = _states(A)
    for step in range(3):
        noise = B.make_noise(opt_name, np.random.default_rng(B.case_seed("terminal-value", opt_name) + step), A, 1, n=N, h=H, iters=iters)
        out = []
        for eng in (a, b):
            eng.set_trace(True)
            if opt_name in ("CEM", "PI2"):                     # unit variance on a range of 0.5: the draws leave the bounds on both sides
                eng.set_state("var0", np.ones((A, H, 1), F))
            _inject(L, eng, opt_name, noise)
            act, nxt, rew = eng.optimize(state)
            out.append((act, nxt, rew, [eng.get_trace(it, L.TRACE_REWARDS) for it in range(n_it)]))
        (act, nxt, rew, tr), (act_t, nxt_t, rew_t, tr_t) = out
        for it, (r, r_t) in enumerate(zip(tr, tr_t)):
            np.testing.assert_allclose(r, r_t, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H, err_msg="step %d iteration %d" % (step, it))
        np.testing.assert_allclose(act, act_t, rtol=0, atol=2e-3, err_msg="step %d" % step)
        np.testing.assert_allclose(nxt, nxt_t, rtol=2e-5, atol=2e-3)
        np.testing.assert_allclose(rew, rew_t, rtol=1e-3, atol=1e-2)          # the record's reward carries no terminal term on either side
        state = nxt_t.astype(F)                                # both go on from the same state


# ---- 4. tiles and agents --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 17, 33])
def test_tiles_against_the_statement(L, N):
    H, w = 3, 1.0
    net = V.small_nets()[4]
    eng = _engine(L, "builtin", A=1, H=H)
    rng = np.random.default_rng(N)
    state, seq = _states(1), rng.uniform(-1, 1, (N, 1, H, 1)).astype(F)
    before = eng.evaluate(state, seq)
    s_last = _last_states(eng, state, seq)
    _set(eng, net, w)
    got = eng.evaluate(state, seq)
    np.testing.assert_allclose(got, V.with_terminal(before, net, w, s_last), rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    np.testing.assert_array_equal(eng.evaluate(state, seq), got)


@pytest.mark.parametrize("kind", KINDS)
def test_agent_split_and_repeat_give_equal_bits(L, kind):
    N, H, w = 37, 5, -0.5
    net = V.small_nets()[1]
    rng = np.random.default_rng(2)
    state4, seq4 = _states(4), rng.uniform(-1, 1, (N, 4, H, 1)).astype(F)
    eng = _engine(L, kind, A=4, H=H)
    _set(eng, net, w)
    full = eng.evaluate(state4, seq4)
    np.testing.assert_array_equal(eng.evaluate(state4, seq4), full)
    for off in (0, 2):
        half = _engine(L, kind, A=2, H=H, agent_offset=off, num_agents_global=4)
        _set(half, net, w)
        np.testing.assert_array_equal(half.evaluate(state4[off:off + 2], np.ascontiguousarray(seq4[:, off:off + 2])), full[:, off:off + 2])


# ---- 5. NaN and refresh ---------------------------------------------------------------------------------------------------------
def test_nan_weights_heal_and_the_weight_alone_changes_the_scores(L):
    N, A, H = 37, 2, 5
    net, other = V.small_nets()[1], V.small_nets()[2]
    eng = _engine(L, "builtin", A=A, H=H, lo=B.NARROW[0], hi=B.NARROW[1])
    rng = np.random.default_rng(3)
    state, seq = _states(A), rng.uniform(-1, 1, (N, A, H, 1)).astype(F)
    before = eng.evaluate(state, seq)
    s_last = _last_states(eng, state, seq)
    bad = [w.copy() for w in net.ws]
    bad[0][0, 0] = np.nan
    eng.set_terminal_value_mlp(bad, net.bs, net.codes(), net.stats, 1.0)
    np.testing.assert_array_equal(eng.evaluate(state, seq), np.full((N, A), F(-1.0e6)))
    _set(eng, other, 1.0)                                      # new finite weights (and no statistics): replaced in place
    one = eng.evaluate(state, seq)
    np.testing.assert_allclose(one, V.with_terminal(before, other, 1.0, s_last), rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    _set(eng, other, -2.0)                                     # only the weight
    two = eng.evaluate(state, seq)
    np.testing.assert_allclose(two.astype(np.float64) - one, -3.0 * V.value(other, s_last).reshape(N, A),
                               rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    assert np.std(two - one) > 0.3


# ---- 6. refusals and codes -------------------------------------------------------------------------------------------------------
def test_refusals_and_error_codes(L):
    from blackbox_mpc_amd.engine import Engine
    net = V.small_nets()[1]
    N, A, H = 8, 1, 3
    state, seq = _states(A), np.random.default_rng(0).uniform(-1, 1, (N, A, H, 1)).astype(F)
    eng = _engine(L, "builtin", A=A, H=H)
    plain = eng.evaluate(state, seq)
    good = (net.ws, net.bs, net.codes(), net.stats, 1.0)

    def usable(want):
        np.testing.assert_array_equal(eng.evaluate(state, seq), want)

    # refused on a handle without a network: it keeps computing what it computed
    deep = [np.zeros((3, 8), F)] + [np.zeros((8, 8), F)] * 7 + [np.zeros((8, 1), F)]
    _raises(L, L.E_UNSUPPORTED, lambda: eng.set_terminal_value_mlp(deep, [np.zeros(w.shape[1], F) for w in deep], [1] * 9, None, 1.0))
    usable(plain)
    wide = [np.zeros((3, 513), F), np.zeros((513, 1), F)]
    _raises(L, L.E_UNSUPPORTED, lambda: eng.set_terminal_value_mlp(wide, [np.zeros(513, F), np.zeros(1, F)], [1, 0], None, 1.0))
    usable(plain)
    _raises(L, L.E_INVALID, lambda: eng.set_terminal_value_mlp([np.zeros((4, 20), F), net.ws[1]], net.bs, net.codes(), None, 1.0))   # dims[0] != S
    usable(plain)
    _raises(L, L.E_INVALID, lambda: eng.set_terminal_value_mlp([net.ws[0], np.zeros((20, 2), F)], [net.bs[0], np.zeros(2, F)], net.codes(), None, 1.0))
    usable(plain)
    _raises(L, L.E_INVALID, lambda: eng.set_terminal_value_mlp(net.ws, net.bs, [1, 99], net.stats, 1.0))
    usable(plain)
    for bad_w in (np.nan, np.inf, -np.inf):
        _raises(L, L.E_INVALID, lambda: eng.set_terminal_value_mlp(net.ws, net.bs, net.codes(), net.stats, bad_w))
    usable(plain)
    import ctypes
    i32 = ctypes.c_int32
    dims, acts = (i32 * 3)(3, 20, 1), (i32 * 2)(1, 0)
    wp = (ctypes.c_void_p * 2)(*[w.ctypes.data for w in net.ws])
    bp = (ctypes.c_void_p * 2)(*[b.ctypes.data for b in net.bs])
    assert L.lib.bbmpc_set_terminal_value_mlp(eng._h, 2, None, acts, wp, bp, 0, None, 1.0) == L.E_INVALID            # NULL pointers
    assert L.lib.bbmpc_set_terminal_value_mlp(eng._h, 2, dims, acts, None, bp, 0, None, 1.0) == L.E_INVALID
    assert L.lib.bbmpc_set_terminal_value_mlp(eng._h, 2, dims, acts, wp, bp, 1, None, 1.0) == L.E_INVALID            # is_normalized without stats
    assert L.lib.bbmpc_evaluate_terminal_value(eng._h, None, 1, None) == L.E_INVALID
    usable(plain)
    # particles, either order
    eng.set_particles(4, np.zeros(3, F), 0.0)
    assert "particles" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_terminal_value_mlp(*good))
    eng.set_particles(0)
    usable(plain)
    eng.set_terminal_value_mlp(*good)
    with_v = eng.evaluate(state, seq)
    assert np.max(np.abs(with_v - plain)) > 0.1
    assert "terminal value" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_particles(4, np.zeros(3, F), 0.0))
    usable(with_v)
    # an inverse target transform, either order
    assert "transform" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_inverse_transform_source(B.XFORM_SOURCE))
    usable(with_v)
    _raises(L, L.E_INVALID, lambda: eng.set_terminal_value_mlp(net.ws, net.bs, [1, 99], net.stats, 1.0))              # a refused replacement keeps the old network
    usable(with_v)
    eng.set_terminal_value_mlp(None, None, None)
    eng.set_inverse_transform_source(B.XFORM_SOURCE)
    with_x = eng.evaluate(state, seq)
    assert "transform" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_terminal_value_mlp(*good))
    usable(with_x)
    # torch-callable plug-ins (device-memory callbacks), either order
    cb = L.ROWS_CALLBACK(lambda *args: 0)
    user = _engine(L, "user", A=A, H=H)
    scored = user.evaluate(state, seq)
    user.set_reward_callback(cb)
    assert "callback" in _raises(L, L.E_UNSUPPORTED, lambda: user.set_terminal_value_mlp(*good))
    user.set_reward_source(RU.MIXED_REWARD)
    np.testing.assert_array_equal(user.evaluate(state, seq), scored)
    user.set_terminal_value_mlp(*good)
    with_u = user.evaluate(state, seq)
    assert "callback" in _raises(L, L.E_UNSUPPORTED, lambda: user.set_reward_callback(cb))
    np.testing.assert_array_equal(user.evaluate(state, seq), with_u)
    # analytic and user dynamics
    pend = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H)
    p0 = pend.evaluate(state, seq)
    assert "BBMPC_DYN_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: pend.set_terminal_value_mlp(*good))
    np.testing.assert_array_equal(pend.evaluate(state, seq), p0)
    udyn = Engine(L.OPT_NONE, L.DYN_USER, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H)
    assert "BBMPC_DYN_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: udyn.set_terminal_value_mlp(*good))


# ---- 7. the Python layer ---------------------------------------------------------------------------------------------------------
def test_python_layer_fits_plans_and_reuploads_a_refitted_value_model(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.policies import RandomPolicy
    from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.dynamics_learning import learn_dynamics_from_policy
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    from blackbox_mpc_amd.utils.rollouts import ModelEnvironment, perform_rollouts, rollout_on_device
    from blackbox_mpc_amd.value_functions import LearnedValueMLP
    act_space, obs_space = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    A, T = 3, 20
    start = O.pendulum_start_states(A)
    true_handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=PendulumTrueModel(), true_model=True)
    env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)
    value = LearnedValueMLP(3, [20, 1], ["tanh", None], seed=1)
    v0 = value._version
    handler = learn_dynamics_from_policy(
        env, RandomPolicy(A, act_space, seed=0), number_of_rollouts=2, task_horizon=T,
        dynamics_function=DeterministicMLP(layers=[4, 16, 3], activation_functions=["tanh", None], seed=0), epochs=2, batch_size=32, seed=0,
        value_model=value, value_n_step=5, value_train_args=dict(epochs=2, batch_size=32, seed=0, gamma=0.95))
    assert value._version > v0 and value.normalization_stats() is not None and len(value._episodes) == 2
    H, N, w = 5, 20, 0.5
    policy = MPCPolicy(reward_function=pendulum_reward_function, env_action_space=act_space, env_observation_space=obs_space,
                       dynamics_handler=handler, optimizer_name="CEM", num_agents=A, planning_horizon=H, population_size=64, num_elite=8,
                       max_iterations=2, terminal_value=value, terminal_weight=w)
    a1, n1, r1 = policy.act(start, 0)
    assert a1.shape == (A, 1) and np.all(np.isfinite(a1)) and np.all(np.isfinite(r1))
    ev = policy._trajectory_evaluator
    plain = DeterministicTrajectoryEvaluator(pendulum_reward_function, handler)
    seq = np.random.default_rng(0).uniform(-2, 2, (N, A, H, 1)).astype(F)

    def statement():
        rows_s = np.broadcast_to(start[None], (N, A, 3)).reshape(N * A, 3)
        states, _ = plain.predict_trajectories(rows_s, seq.reshape(N * A, H, 1))
        term = w * value(states[:, -1]).astype(np.float64).reshape(N, A)
        return plain(start, seq).astype(np.float64) + term, term
    first = ev(start, seq)
    want, term = statement()
    assert np.std(term) > 0.01
    np.testing.assert_allclose(first, want, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    # the record is the step's own: no terminal term in it
    np.testing.assert_allclose(r1, plain.evaluate_next_reward(start, n1, a1), rtol=2e-5, atol=2e-5)
    traj_obs, _, traj_rews = perform_rollouts(env, 1, T, RandomPolicy(A, act_space, seed=1))
    value.train_on_rollouts(traj_obs, traj_rews, 5, gamma=0.95, bootstrap=True, epochs=3, batch_size=32, seed=0, device="cpu")
    value.set_weights([wt * F(-1.5) for wt in value.weights], [b + F(0.25) for b in value.biases])     # ... and visibly different
    policy.act(start, 1)                                       # the optimizer's engine uploads the new weights before it plans
    assert policy._optimizer._engine._val_version == value._version
    second = ev(start, seq)
    want2, _ = statement()
    assert np.max(np.abs(second - first)) > 0.05
    np.testing.assert_allclose(second, want2, rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)
    np.testing.assert_allclose(policy._optimizer._engine.evaluate_terminal_value(start), value(start), rtol=2e-5, atol=2e-5)
    acts, obs, rews = rollout_on_device(policy, start, 3)
    assert acts.shape[0] == 3 and np.all(np.isfinite(rews))
