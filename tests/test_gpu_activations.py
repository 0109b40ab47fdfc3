"""The Keras activation set in the learned-model kernels (reference dynamics_functions/deterministic_mlp.py:19-24) on the
GPU: the accuracy of every form (csrc/activations.hpp) through the row kernel, rollouts on every kernel family that takes
run-time activations against a float64 oracle network, the one-step paths, an optimizer in lock-step, MPCPolicy end to end
from a saved model, and GPU training against the host trainer.

Tolerances as tests/test_gpu_mlp.py: single model step rtol 2e-5 + atol 2e-5; H-step rewards rtol 1e-3 + atol 1e-3 * H."""
import numpy as np
import pytest

from tests.parity_util import assert_cheetah_rewards, cheetah_threshold_margin
from tests.test_gpu_mlp import _lockstep_select

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
F = np.float32
NEW = ["elu", "selu", "softplus", "softsign", "exponential", "hard_sigmoid", "swish", "leaky_relu", "relu6"]
CODE = {None: 0, "tanh": 1, "relu": 2, "sigmoid": 3, "elu": 4, "selu": 5, "softplus": 6, "softsign": 7, "exponential": 8,
        "hard_sigmoid": 9, "swish": 10, "leaky_relu": 11, "relu6": 12}
SELU_A, SELU_L = 1.6732632423543772, 1.0507009873554805


def act64(name, x):
    """the TF 2.0 definition in float64, with the limits at +-inf and NaN passed through"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if name is None:
            return x
        if name == "tanh":
            return np.tanh(x)
        if name == "relu":
            return np.maximum(x, 0.0)
        if name == "sigmoid":
            return 0.5 * (1.0 + np.tanh(0.5 * x))
        if name == "elu":
            return np.where(x > 0, x, np.expm1(x))
        if name == "selu":
            return SELU_L * np.where(x > 0, x, SELU_A * np.expm1(x))
        if name == "softplus":
            return np.logaddexp(0.0, x)
        if name == "softsign":
            return np.where(np.isinf(x), np.sign(x), x / (1.0 + np.abs(x)))
        if name == "exponential":
            return np.exp(x)
        if name == "hard_sigmoid":
            return np.clip(0.2 * x + 0.5, 0.0, 1.0)
        if name == "swish":
            return np.where(np.isneginf(x), 0.0, x * 0.5 * (1.0 + np.tanh(0.5 * x)))
        if name == "leaky_relu":
            return np.where(x >= 0, x, 0.2 * x)
        if name == "relu6":
            return np.clip(x, 0.0, 6.0)
    raise ValueError(name)


class MLP64:
    """DeterministicMLP.__call__ (deterministic_mlp.py:27-51) for the oracle's Handler: the products summed in float64 and
    rounded once (as oracle_np.MLP), the activation evaluated in float64 on the float32 pre-activation and rounded"""

    def __init__(self, weights, biases, acts):
        self.weights = [np.asarray(w, F) for w in weights]
        self.biases = [np.asarray(b, F) for b in biases]
        self.acts = list(acts)

    def __call__(self, x):
        x = np.asarray(x, F)
        for w, b, a in zip(self.weights, self.biases, self.acts):
            y = (x.astype(np.float64) @ w.astype(np.float64)).astype(F)
            y = (y + b).astype(F)
            x = act64(a, y).astype(F)
        return x


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _stats(S, U, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 0.2, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F),
            rng.normal(0, 0.1, U).astype(F), rng.uniform(0.5, 1.5, U).astype(F),
            rng.normal(0, 0.01, S).astype(F), rng.uniform(0.05, 0.15, S).astype(F)]


def _params(dims, acts, seed=42):
    ws, bs = O.make_mlp_params(dims, seed=seed)
    rng = np.random.default_rng(seed + 1)
    bs = [rng.normal(0, 0.05, b.shape).astype(F) for b in bs]
    if "exponential" in acts:          # e^x stacked on e^x: keep the pre-activations O(1)
        ws = [(w * F(0.3)).astype(F) for w in ws]
    return ws, bs


# ---- the forms, through the row kernel (bbmpc_mlp_forward) -------------------------------------------------------------
@pytest.mark.parametrize("name", NEW + ["tanh", "sigmoid"])
def test_each_form_against_float64(L, name):
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    # one Dense layer [x | u] -> x with kernel [I; 0] and zero bias: the layer output is act(x) (one input per row, so an
    # infinite x meets no 0 * inf)
    m = DeterministicMLP([2, 1], [name])
    m.set_weights([np.array([[1.0], [0.0]], F)], [np.zeros(1, F)])
    sweep = np.linspace(-30.0, 30.0, 240001).astype(F)
    fine = np.linspace(-3.0, 3.0, 60001).astype(F)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-30, -1e-30, 88.0, 88.8, -88.0, -104.0, 1e6, -1e6], F)
    x = np.concatenate([sweep, fine, special])
    got = m(np.stack([x, np.zeros_like(x)], 1))[:, 0].astype(np.float64)
    want = act64(name, x.astype(np.float64))
    assert np.array_equal(np.isnan(got), np.isnan(want)), x[np.isnan(got) != np.isnan(want)]
    inf = np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf])
    ok = ~np.isnan(want) & ~inf
    # exponential overflows float32 beyond ~88.72 where float64 does not: the float32 limit is +inf
    f32_over = ok & (np.abs(want) > np.finfo(F).max)
    assert np.all(np.isposinf(got[f32_over]))
    ok &= ~f32_over
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    assert err.max() <= 1e-6, (name, float(err.max()), float(x[ok][np.argmax(err)]))
    # the limits at +-inf
    lim = {"elu": (np.inf, -1.0), "selu": (np.inf, -SELU_L * SELU_A), "softplus": (np.inf, 0.0), "softsign": (1.0, -1.0),
           "exponential": (np.inf, 0.0), "hard_sigmoid": (1.0, 0.0), "swish": (np.inf, 0.0), "leaky_relu": (np.inf, -np.inf),
           "relu6": (6.0, 0.0), "tanh": (1.0, -1.0), "sigmoid": (1.0, 0.0)}[name]
    i = len(sweep) + len(fine)
    np.testing.assert_allclose([got[i + 2], got[i + 3]], lim, rtol=1e-6, atol=1e-6)


def test_codes_out_of_range_are_invalid(L):
    from blackbox_mpc_amd.engine import Engine
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_USER, [-1.0], [1.0], dim_s=3, num_agents=1, planning_horizon=1)
    ws, bs = O.make_mlp_params([4, 8, 3])
    for bad in (13, -1):
        with pytest.raises(L.BBMPCError) as ei:
            eng.set_mlp(ws, bs, [bad, 0])
        assert ei.value.code == L.E_INVALID
    eng.set_mlp(ws, bs, [12, 4])       # the last valid code, on either layer


# ---- rollouts on every kernel family with run-time activations ---------------------------------------------------------
Q4S_USER_REWARD = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    float r = 0.0f;
    for (int s = 0; s < S; ++s) r = r + (nxt[s] - cur[s]) * (0.25f + 0.125f * (float)(s & 3));
    for (int u = 0; u < U; ++u) r = r - 0.0625f * (act[u] * act[u]);
    return r;
}
"""


def _user_reward_np(cur, act, nxt):
    S, U = cur.shape[1], act.shape[1]
    r = np.zeros(cur.shape[0], F)
    for s in range(S):
        r = (r + ((nxt[:, s] - cur[:, s]).astype(F) * F(0.25 + 0.125 * (s & 3))).astype(F)).astype(F)
    for u in range(U):
        r = (r - (F(0.0625) * (act[:, u] * act[:, u]).astype(F)).astype(F)).astype(F)
    return r


XFORM_DEFAULT = ("__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {\n"
                 "    for (int i = 0; i < S; ++i) next[i] = cur[i] + dev[i];\n}\n")

# (id, dims, "h" = the activation on the hidden layers / "a" = on every layer, reward, env switches, kernel, N, H)
ROLL = [
    ("q4s", [26, 200, 200, 20], "h", "cheetah", {"BBMPC_MLP_Q4": "1"}, "k_rollout_mlp_q4s", 64, 12),
    ("q4s_256", [26, 256, 256, 20], "h", "cheetah", {"BBMPC_MLP_Q4": "1"}, "k_rollout_mlp_q4s", 64, 12),
    ("q4s_dimS17", [23, 200, 200, 17], "h", "user", {"BBMPC_MLP_Q4": "1"}, "k_rollout_mlp_q4s", 64, 12),
    ("q4s_dimS18_last", [24, 200, 200, 18], "a", "cheetah", {"BBMPC_MLP_Q4": "1"}, "k_rollout_mlp_q4s", 64, 12),
    ("generic_deep", [26, 500, 500, 500, 20], "h", "cheetah", {}, "k_rollout_mlp", 48, 6),
    ("generic_half_tile", [23, 40, 18], "h", "cheetah", {"BBMPC_MLP_GENERIC": "1"}, "k_rollout_mlp", 77, 12),
    ("generic_half_tile_last", [23, 40, 18], "a", "cheetah", {"BBMPC_MLP_GENERIC": "1"}, "k_rollout_mlp", 77, 12),
    ("w4", [4, 32, 32, 3], "h", "pendulum", {}, "k_rollout_mlp_w4", 77, 20),
    ("w4_padded_last", [4, 24, 20, 3], "a", "pendulum", {}, "k_rollout_mlp_w4", 77, 20),
    ("wave", [4, 32, 32, 3], "h", "pendulum", {"BBMPC_MLP_W4": "0"}, "k_rollout_mlp_wave", 77, 20),
    ("wave_padded_last", [4, 40, 40, 3], "a", "pendulum", {"BBMPC_MLP_W4": "0"}, "k_rollout_mlp_wave", 77, 20),
    ("xform", [26, 200, 200, 20], "h", "cheetah", {}, "bbmpc_mlp_xform_rollout(hiprtc)", 64, 12),
]


@pytest.mark.parametrize("case", ROLL, ids=[c[0] for c in ROLL])
@pytest.mark.parametrize("name", NEW)
def test_rollouts_match_the_float64_network(L, monkeypatch, name, case):
    from blackbox_mpc_amd.engine import Engine
    cid, dims, where, reward, env, kernel, N, H = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S, U = dims[-1], dims[0] - dims[-1]
    acts = [name] * (len(dims) - 1) if where == "a" else [name] * (len(dims) - 2) + [None]
    A = 2
    ws, bs = _params(dims, acts)
    stats = _stats(S, U, 7)
    lim = 2.0 if reward == "pendulum" else 1.0
    rk = {"cheetah": L.REW_CHEETAH, "pendulum": L.REW_PENDULUM, "user": L.REW_USER}[reward]
    eng = Engine(L.OPT_NONE, L.DYN_MLP, rk, [-lim] * U, [lim] * U, dim_s=S, num_agents=A, planning_horizon=H)
    if reward == "user":
        eng.set_reward_source(Q4S_USER_REWARD)
    eng.set_mlp(ws, bs, [CODE[a] for a in acts], stats)
    if cid == "xform":
        eng.set_inverse_transform_source(XFORM_DEFAULT)
    ev = O.Evaluator(_user_reward_np if reward == "user" else reward, O.Handler(MLP64(ws, bs, acts), False, True, stats))
    rng = np.random.default_rng(len(dims) * 100 + S)
    states = O.pendulum_start_states(A) if reward == "pendulum" else rng.normal(0, 0.3, (A, S)).astype(F)
    seq = rng.uniform(-lim, lim, (N, A, H, U)).astype(F)
    eng.set_profiling(True)
    got = eng.evaluate(states, seq)
    assert eng.get_profile()[2] == kernel
    if kernel == "k_rollout_mlp_q4s":     # the instantiation for the extended set (run-time code -2)
        assert ", 7, -2, -2, -2, " in eng.profile_instantiation()
    want = ev(states, seq)
    assert np.all(np.isfinite(want))
    if reward == "cheetah":
        assert_cheetah_rewards(got, want, 1e-3, 1e-3 * H, margin=lambda: cheetah_threshold_margin(ev, states, seq))
    else:
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)


# ---- one-step paths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_one_step_paths(L, name):
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.engine import Engine
    S, U = 20, 6
    dims, acts = [S + U, 200, 200, S], [name, name, name]
    ws, bs = _params(dims, acts)
    stats = _stats(S, U, 3)
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_CHEETAH, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=1, planning_horizon=1)
    eng.set_mlp(ws, bs, [CODE[a] for a in acts], stats)
    ev = O.Evaluator("cheetah", O.Handler(MLP64(ws, bs, acts), False, True, stats))
    rng = np.random.default_rng(1)
    s = rng.normal(0, 0.5, (333, S)).astype(F)
    a = rng.uniform(-1, 1, (333, U)).astype(F)
    nxt_o = ev.predict_next_state(s, a)
    np.testing.assert_allclose(eng.predict_next_state(s, a), nxt_o, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(eng.evaluate_next_reward(s, nxt_o, a), ev.evaluate_next_reward(s, nxt_o, a), rtol=2e-5,
                               atol=2e-5)
    m = DeterministicMLP(dims, acts)
    m.set_weights(ws, bs)
    x = np.concatenate([s, a], 1)
    np.testing.assert_allclose(m(x), MLP64(ws, bs, acts)(x), rtol=2e-5, atol=2e-5)


# ---- an optimizer in lock-step, then MPCPolicy from a saved model ------------------------------------------------------
def test_cem_with_a_swish_network_lockstep(L):
    from blackbox_mpc_amd.engine import Engine
    S, U, N, A, H, iters, k = 20, 6, 96, 2, 8, 2, 12
    dims, acts = [S + U, 200, 200, S], ["swish", "swish", None]
    ws, bs = _params(dims, acts)
    stats = _stats(S, U, 5)
    eng = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_CHEETAH, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=A, planning_horizon=H,
                 population_size=N, max_iterations=iters, num_elite=k)
    eng.set_mlp(ws, bs, [CODE[a] for a in acts], stats)
    ev = O.Evaluator("cheetah", O.Handler(MLP64(ws, bs, acts), False, True, stats))
    eng.set_trace(True)
    rng = np.random.default_rng(N)
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, U)) for _ in range(iters)]}
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    states = O.cheetah_start_states(A, S)
    act, nxt, rew = eng.optimize(states)

    cem = O.CEM(ev, [-1.0] * U, [1.0] * U, horizon=H, max_iterations=iters, population=N, num_elite=k, num_agents=A)
    cem._optimize(states, noise, forced_elites=_lockstep_select(L, eng, A, k, iters, 1e-3, 1e-3 * H))
    for it in range(iters):
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), cem.trace[it]["mean"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_VAR), cem.trace[it]["var"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(act, cem.trace[-1]["mean"][:, 0], rtol=0, atol=1e-4)
    nxt_o = ev.predict_next_state(states, act)
    np.testing.assert_allclose(nxt, nxt_o, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("name", ["swish", "elu", "softplus"])
def test_mpc_policy_from_a_saved_model(L, tmp_path, name):
    from blackbox_mpc_amd.dynamics_functions import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.utils.cheetah import reward_function
    S, U = 20, 6
    act_space, obs_space = Box([-1.0] * U, [1.0] * U), Box([-10.0] * S, [10.0] * S)
    acts = [name, name, None]
    mlp = DeterministicMLP(layers=[S + U, 200, 200, S], activation_functions=acts, seed=1)
    ws, bs = _params([S + U, 200, 200, S], acts)
    mlp.set_weights(ws, bs)
    h = SystemDynamicsHandler(act_space, obs_space, dynamics_function=mlp, true_model=False, is_normalized=True)
    stats = _stats(S, U, 9)
    h.set_normalization_stats(*stats)
    h.save(str(tmp_path))
    h2 = SystemDynamicsHandler(act_space, obs_space, true_model=False, is_normalized=True, saved_model_dir=str(tmp_path))
    assert h2._dynamics_function.activation_codes == [CODE[a] for a in acts]
    pol = MPCPolicy(reward_function=reward_function, env_action_space=act_space, env_observation_space=obs_space,
                    dynamics_handler=h2, optimizer_name="CEM", num_agents=2, planning_horizon=10, population_size=128,
                    max_iterations=2, num_elite=16)
    obs = O.cheetah_start_states(2, S)
    a, n, r = pol.act(obs, 0)
    assert a.shape == (2, U) and np.all(np.isfinite(a)) and np.all(np.isfinite(r))
    np.testing.assert_array_equal(n, pol._trajectory_evaluator.predict_next_state(obs, a))
    ev = O.Evaluator("cheetah", O.Handler(MLP64(ws, bs, acts), False, True, stats))
    np.testing.assert_allclose(n, ev.predict_next_state(obs, a), rtol=2e-5, atol=2e-5)


# ---- training on the GPU against the host trainer ----------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("name", ["swish", "elu", "hard_sigmoid"])
def test_gpu_training_matches_the_host_trainer(L, monkeypatch, graph, name):
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer
    monkeypatch.setenv("BBMPC_TRAIN_GRAPH", graph)
    dims, acts = [4, 64, 64, 3], [name, name, None]
    ws, bs = _params(dims, acts, seed=3)
    rng = np.random.default_rng(4)
    tin = rng.normal(0, 1, (600, 4)).astype(F)
    tout = np.tanh(tin[:, :3] * 0.7 + tin[:, 3:] * 0.3).astype(F)
    vin = rng.normal(0, 1, (128, 4)).astype(F)
    vout = np.tanh(vin[:, :3] * 0.7 + vin[:, 3:] * 0.3).astype(F)
    epochs, B = 5, 32
    perms = [rng.permutation(600) for _ in range(epochs)]
    codes = [CODE[a] for a in acts]
    res = {}
    for dev in ("cuda", "cpu"):
        tr = DenseTrainer(ws, bs, codes, dev, learning_rate=2e-3)
        tl, vl = tr.fit(tin, tout, vin, vout, epochs, B, permutations=perms)
        res[dev] = (tr.numpy_params(), tl, vl)
    (wg, bg), tlg, vlg = res["cuda"]
    (wc, bc), tlc, vlc = res["cpu"]
    for got, want in zip(wg + bg, wc + bc):
        np.testing.assert_allclose(got, want, rtol=0, atol=3e-4)
    np.testing.assert_allclose(tlg, tlc, rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(vlg, vlc, rtol=2e-4, atol=1e-6)
    assert tlg[-1] < tlg[0]
