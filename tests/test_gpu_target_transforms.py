"""Custom inverse target transforms on the GPU (reference dynamics_handlers/system_dynamics_handler.py:128-161):
the learned-model rollout with a HipInverseTargetTransform inlined (kernels_mlp_xform.hpp, hiprtc) and its step-wise twin
(BBMPC_USER_STEPWISE=1) against the NumPy oracle with the same transform, the optimizers, the one-step paths, the
HIP-source true model, and training targets from a HipTargetTransform."""
import numpy as np
import pytest

from oracle import oracle_np as O
from oracle import oracle_train as OT

pytestmark = pytest.mark.gpu

F = np.float32
PI, TWO_PI = F(3.14159274101257324), F(6.28318548202514648)

XFORMS = {
    # next = dev + state: the default, restated
    "default": ("for (int i = 0; i < S; ++i) next[i] = cur[i] + dev[i];",
                lambda s, d: (s + d).astype(F)),
    # the model predicts the next state itself
    "absolute": ("for (int i = 0; i < S; ++i) next[i] = dev[i];",
                 lambda s, d: d.copy()),
    # a scaled delta
    "scaled": ("for (int i = 0; i < S; ++i) next[i] = cur[i] + 0.5f * dev[i];",
               lambda s, d: (s + (F(0.5) * d).astype(F)).astype(F)),
    # a delta whose coordinate 0 is an angle wrapped back into [-pi, pi)
    "wrap": ("for (int i = 0; i < S; ++i) next[i] = cur[i] + dev[i];\n"
             "    const float v = next[0];\n"
             "    next[0] = v - 6.28318548202514648f * floorf((v + 3.14159274101257324f) / 6.28318548202514648f);",
             None),
}


def _wrap(s, d):
    n = (s + d).astype(F)
    v = n[:, 0]
    n[:, 0] = (v - (TWO_PI * np.floor(((v + PI).astype(F) / TWO_PI).astype(F))).astype(F)).astype(F)
    return n


XFORMS["wrap"] = (XFORMS["wrap"][0], _wrap)


def xform_source(name):
    return ("__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {\n"
            "    %s\n}\n" % XFORMS[name][0])


SMOOTH_REWARD = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    float r = 0.0f;
    for (int i = 0; i < S; ++i) r = r - 0.01f * (nxt[i] * nxt[i]);
    for (int u = 0; u < U; ++u) r = r - 0.1f * (act[u] * act[u]);
    return r;
}
"""


def smooth_reward(cur, act, nxt):
    r = np.zeros(cur.shape[0], F)
    for i in range(nxt.shape[1]):
        r = (r - (F(0.01) * (nxt[:, i] * nxt[:, i]).astype(F)).astype(F)).astype(F)
    for u in range(act.shape[1]):
        r = (r - (F(0.1) * (act[:, u] * act[:, u]).astype(F)).astype(F)).astype(F)
    return r


class XformHandler(O.Handler):
    """the oracle handler with a custom inverse transform applied to the de-normalised output (:148-161)"""

    def __init__(self, inverse, *args, **kw):
        super().__init__(*args, **kw)
        self.inverse = inverse

    def process_output(self, s, raw):
        s, raw = O.f32(s), O.f32(raw)
        if self.true_model or not self.is_normalized:
            dev = raw
        else:
            dev = (self.mean_t + (raw * (self.std_t + F(1e-7)).astype(F)).astype(F)).astype(F)
        return self.inverse(s, dev)


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


@pytest.fixture(params=["fused", "stepwise"])
def form(request, monkeypatch):
    if request.param == "stepwise":
        monkeypatch.setenv("BBMPC_USER_STEPWISE", "1")
    else:
        monkeypatch.delenv("BBMPC_USER_STEPWISE", raising=False)
    yield request.param


ACT_CODE = {"tanh": 1, "relu": 2, None: 0}
NETS = {
    "cheetah": ([26, 200, 200, 20], ["tanh", "tanh", None]),
    "pendulum": ([4, 32, 32, 32, 3], ["relu", "relu", "relu", None]),
    "deep": ([26, 96, 96, 96, 96, 96, 20], ["tanh", "relu", "tanh", "relu", "tanh", None]),
}


def _stats(S, U, normalized):
    if not normalized:
        return None
    rng = np.random.default_rng(S + U)
    return [rng.uniform(-0.1, 0.1, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F), rng.uniform(-0.1, 0.1, U).astype(F),
            rng.uniform(0.5, 1.5, U).astype(F), rng.uniform(-0.01, 0.01, S).astype(F), np.full(S, 0.1, F)]


def _engine(L, net, reward, xform, A, H, normalized, opt=None, **kw):
    from blackbox_mpc_amd.engine import Engine
    dims, acts = NETS[net]
    S, U = dims[-1], dims[0] - dims[-1]
    ws, bs = O.make_mlp_params(dims, seed=42)
    stats = _stats(S, U, normalized)
    lo, hi = ([-2.0], [2.0]) if U == 1 else ([-1.0] * U, [1.0] * U)
    eng = Engine(L.OPT_NONE if opt is None else opt, L.DYN_MLP, reward, lo, hi, dim_s=S, num_agents=A, planning_horizon=H, **kw)
    eng.set_mlp(ws, bs, [ACT_CODE[a] for a in acts], stats)
    if reward == L.REW_USER:
        eng.set_reward_source(SMOOTH_REWARD)
    if xform is not None:
        eng.set_inverse_transform_source(xform_source(xform))
    return eng, (ws, bs, acts, stats, S, U)


def _start(S, A):
    return O.pendulum_start_states(A) if S == 3 else O.cheetah_start_states(A, S)


def _oracle(spec, reward, xform):
    ws, bs, acts, stats, S, U = spec
    h = XformHandler(XFORMS[xform][1], O.MLP(ws, bs, acts), False, stats is not None, stats)
    return O.Evaluator(reward, h)


def test_default_equivalent_transform_matches_the_builtin_path(L, form, monkeypatch):
    A, H, N = 2, 12, 300
    eng, spec = _engine(L, "cheetah", L.REW_CHEETAH, "default", A, H, True)
    monkeypatch.delenv("BBMPC_USER_STEPWISE", raising=False)
    ref, _ = _engine(L, "cheetah", L.REW_CHEETAH, None, A, H, True)
    states = _start(20, A)
    seq = np.random.default_rng(7).uniform(-1, 1, (N, A, H, 6)).astype(F)
    got = eng.evaluate(states, seq)
    want = O.Evaluator("cheetah", O.Handler(O.MLP(spec[0], spec[1], spec[2]), False, True, spec[3]))(states, seq)
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)
    np.testing.assert_allclose(got, ref.evaluate(states, seq), rtol=1e-3, atol=1e-3 * H)
    # the final states: predict_next_state walks the same rows
    a0 = seq[:4, 0, 0]
    np.testing.assert_allclose(eng.predict_next_state(np.repeat(states[:1], 4, 0), a0),
                               ref.predict_next_state(np.repeat(states[:1], 4, 0), a0), rtol=1e-5, atol=1e-6)


def test_fused_and_stepwise_forms_agree(L, monkeypatch):
    A, H, N = 2, 12, 300
    monkeypatch.delenv("BBMPC_USER_STEPWISE", raising=False)
    fused, _ = _engine(L, "cheetah", L.REW_USER, "scaled", A, H, True)
    fused.set_profiling(True)
    monkeypatch.setenv("BBMPC_USER_STEPWISE", "1")
    step, _ = _engine(L, "cheetah", L.REW_USER, "scaled", A, H, True)
    states = _start(20, A)
    seq = np.random.default_rng(3).uniform(-1, 1, (N, A, H, 6)).astype(F)
    got = fused.evaluate(states, seq)
    assert fused.get_profile()[2] == "bbmpc_mlp_xform_rollout(hiprtc)"
    want = step.evaluate(states, seq)
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5 * float(np.abs(want).max()))


CASES = [  # (network, transform, normalised, A, H)
    ("cheetah", "absolute", True, 1, 30),
    ("cheetah", "wrap", False, 4, 1),
    ("cheetah", "scaled", True, 4, 30),
    ("pendulum", "absolute", False, 4, 30),
    ("pendulum", "wrap", True, 1, 30),
    ("pendulum", "scaled", False, 1, 1),
    ("deep", "absolute", True, 4, 1),
    ("deep", "wrap", True, 1, 30),
    ("deep", "scaled", False, 4, 30),
]


@pytest.mark.parametrize("net,xform,normalized,A,H", CASES)
def test_custom_transforms_match_the_oracle(L, form, net, xform, normalized, A, H):
    reward = L.REW_PENDULUM if net == "pendulum" else L.REW_USER
    eng, spec = _engine(L, net, reward, xform, A, H, normalized)
    S, U = spec[4], spec[5]
    ev = _oracle(spec, "pendulum" if net == "pendulum" else smooth_reward, xform)
    rng = np.random.default_rng(11)
    states = _start(S, A)
    lim = 2.0 if U == 1 else 1.0
    seq = rng.uniform(-lim, lim, (200, A, H, U)).astype(F)
    np.testing.assert_allclose(eng.evaluate(states, seq), ev(states, seq), rtol=1e-3, atol=1e-3 * H)
    a = rng.uniform(-lim, lim, (5, U)).astype(F)
    s5 = np.repeat(states[:1], 5, 0)
    np.testing.assert_allclose(eng.predict_next_state(s5, a), ev.predict_next_state(s5, a), rtol=1e-4, atol=1e-5)


def _lockstep_select(L, eng, A, k, iters, rtol, atol):
    """the oracle CEM takes the device's elites where two near-tied rewards swap at the elite boundary"""
    hip_el = [eng.get_trace(it, L.TRACE_ELITES) for it in range(iters)]
    hip_r = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(iters)]

    def select(it, r_o, own):
        np.testing.assert_allclose(hip_r[it], r_o, rtol=rtol, atol=atol)
        for a in range(A):
            he = hip_el[it][a]
            if set(own[a]) != set(he):
                kth = np.sort(r_o[:, a])[::-1][k - 1]
                for n in set(own[a]) ^ set(he):
                    assert abs(r_o[n, a] - kth) <= 2 * (atol + rtol * abs(kth)), "elite sets differ beyond the tie tolerance"
        return hip_el[it]
    return select


@pytest.mark.parametrize("xform", ["scaled", "wrap"])
def test_cem_with_a_transform_in_lockstep_with_the_oracle(L, form, xform):
    # CEM with injected draws against the oracle CEM driven by the transformed evaluator
    A, H, N, iters, k = 2, 10, 160, 3, 16
    eng, spec = _engine(L, "cheetah", L.REW_USER, xform, A, H, True, opt=L.OPT_CEM, population_size=N,
                        max_iterations=iters, num_elite=k, seed=5)
    ev = _oracle(spec, smooth_reward, xform)
    eng.set_trace(True)
    rng = np.random.default_rng(21)
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 6)) for _ in range(iters)]}
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    states = _start(20, A)
    act, nxt, rew = eng.optimize(states)
    lo, hi = np.full(6, -1.0, F), np.full(6, 1.0, F)
    cem = O.CEM(ev, lo, hi, horizon=H, max_iterations=iters, population=N, num_elite=k, num_agents=A)
    cem._optimize(states, noise, forced_elites=_lockstep_select(L, eng, A, k, iters, 1e-3, 1e-3 * H))
    for it in range(iters):
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), cem.trace[it]["mean"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(act, cem.trace[-1]["mean"][:, 0], rtol=0, atol=1e-4)
    nxt_o = ev.predict_next_state(states, act)
    np.testing.assert_allclose(nxt, nxt_o, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rew, ev.evaluate_next_reward(states, nxt_o, act), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("opt_name", ["RandomSearch", "CEM", "PI2", "PSO", "SPSA", "CMA-ES"])
def test_optimizers_walk_in_step_with_the_stepwise_twin(L, monkeypatch, opt_name):
    opt = {"RandomSearch": L.OPT_RANDOM_SEARCH, "CEM": L.OPT_CEM, "PI2": L.OPT_PI2, "PSO": L.OPT_PSO, "SPSA": L.OPT_SPSA,
           "CMA-ES": L.OPT_CMAES}[opt_name]
    A, H = 2, 10
    kw = dict(population_size=160, max_iterations=3, num_elite=16, seed=31, lamda=1.0)
    monkeypatch.delenv("BBMPC_USER_STEPWISE", raising=False)
    fused, _ = _engine(L, "pendulum", L.REW_PENDULUM, "scaled", A, H, True, opt=opt, **kw)
    monkeypatch.setenv("BBMPC_USER_STEPWISE", "1")
    step, _ = _engine(L, "pendulum", L.REW_PENDULUM, "scaled", A, H, True, opt=opt, **kw)
    fused.reset()
    step.reset()
    s_f = s_s = _start(3, A)
    tol = 5e-3 if opt_name == "CMA-ES" else 2e-3
    for t in range(3):
        a_f, n_f, r_f = fused.optimize(s_f, t)
        a_s, n_s, r_s = step.optimize(s_s, t)
        assert np.all(np.isfinite(a_f)) and np.all(np.isfinite(n_f))
        np.testing.assert_allclose(a_f, a_s, rtol=0, atol=tol)
        np.testing.assert_allclose(n_f, n_s, rtol=0, atol=tol)
        np.testing.assert_allclose(r_f, r_s, rtol=1e-3, atol=1e-2)
        s_f, s_s = n_f, n_s


@pytest.mark.parametrize("reward", ["builtin", "user"])
def test_act_returns_what_the_one_step_calls_compute(L, form, reward):
    A, H = 3, 8
    rk = L.REW_CHEETAH if reward == "builtin" else L.REW_USER
    eng, spec = _engine(L, "cheetah", rk, "wrap", A, H, True, opt=L.OPT_CEM, population_size=64, max_iterations=2,
                        num_elite=8, seed=9)
    eng.reset()
    s = _start(20, A)
    for t in range(2):
        a, n, r = eng.optimize(s, t)
        np.testing.assert_array_equal(n, eng.predict_next_state(s, a))
        np.testing.assert_array_equal(r, eng.evaluate_next_reward(s, n, a))
        np.testing.assert_allclose(n, _oracle(spec, "cheetah", "wrap").predict_next_state(s, a), rtol=1e-4, atol=1e-5)
        s = n


def _mlp_handler(inverse, normalized=True):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    dims, acts = NETS["cheetah"]
    ws, bs = O.make_mlp_params(dims, seed=42)
    fn = DeterministicMLP(dims, acts, seed=0)
    fn.set_weights(ws, bs)
    h = SystemDynamicsHandler(Box(low=[-1.0] * 6, high=[1.0] * 6), Box(low=[-10.0] * 20, high=[10.0] * 20),
                              dynamics_function=fn, is_normalized=normalized, inverse_transform_targets_func=inverse)
    stats = _stats(20, 6, normalized)
    if normalized:
        h.set_normalization_stats(*stats)
    return h, (ws, bs, acts, stats, 20, 6)


def test_evaluator_api_with_hip_and_torch_rewards(L, form):
    import torch
    from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.device_functions import HipInverseTargetTransform, HipRewardFunction
    h, spec = _mlp_handler(HipInverseTargetTransform(xform_source("absolute")))
    ev = _oracle(spec, smooth_reward, "absolute")
    states = _start(20, 2)
    seq = np.random.default_rng(5).uniform(-1, 1, (64, 2, 6, 6)).astype(F)
    want = ev(states, seq)
    got = DeterministicTrajectoryEvaluator(HipRewardFunction(SMOOTH_REWARD), h)(states, seq)
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=6e-3)

    def torch_smooth(cur, act, nxt):
        return -0.01 * (nxt * nxt).sum(dim=1) - 0.1 * (act * act).sum(dim=1)
    got_t = DeterministicTrajectoryEvaluator(torch_smooth, h)(states, seq)          # a callback reward: step-wise
    np.testing.assert_allclose(got_t, want, rtol=1e-3, atol=6e-3)
    assert torch.cuda.is_available()


USER_DYNAMICS = """
__device__ void bbmpc_user_dynamics(const float* x, float* delta, int S, int U) {
    for (int i = 0; i < S; ++i) delta[i] = 0.05f * x[(i + 1) % S] + 0.1f * x[S];
}
"""


def test_hip_true_model_with_an_inverse_transform(L, form):
    from blackbox_mpc_amd.engine import Engine
    S, U, A, H, N = 3, 1, 2, 15, 150

    def dyn(x):
        d = np.empty((x.shape[0], S), F)
        for i in range(S):
            d[:, i] = ((F(0.05) * x[:, (i + 1) % S]).astype(F) + (F(0.1) * x[:, S]).astype(F)).astype(F)
        return d

    for xform in ("scaled", "absolute"):
        eng = Engine(L.OPT_NONE, L.DYN_USER, L.REW_USER, [-2.0], [2.0], dim_s=S, num_agents=A, planning_horizon=H)
        eng.set_inverse_transform_source(xform_source(xform))          # before the model: its kernels pick it up
        eng.set_dynamics_source(USER_DYNAMICS)
        eng.set_reward_source(SMOOTH_REWARD)
        ev = O.Evaluator(smooth_reward, XformHandler(XFORMS[xform][1], dyn, True))
        states = O.pendulum_start_states(A)
        seq = np.random.default_rng(2).uniform(-2, 2, (N, A, H, U)).astype(F)
        np.testing.assert_allclose(eng.evaluate(states, seq), ev(states, seq), rtol=2e-4, atol=2e-3)
        a = seq[:5, 0, 0]
        s5 = np.repeat(states[:1], 5, 0)
        np.testing.assert_allclose(eng.predict_next_state(s5, a), ev.predict_next_state(s5, a), rtol=1e-5, atol=1e-6)
        eng.set_inverse_transform_source(None)                          # cleared: back to next = delta + state
        ev0 = O.Evaluator(smooth_reward, O.Handler(dyn, True))
        np.testing.assert_allclose(eng.evaluate(states, seq), ev0(states, seq), rtol=2e-4, atol=2e-3)


def test_direct_calls_of_the_transforms(L):
    from blackbox_mpc_amd.utils.device_functions import HipInverseTargetTransform, HipTargetTransform
    rng = np.random.default_rng(0)
    s, d = rng.normal(size=(37, 20)).astype(F), rng.normal(size=(37, 20)).astype(F)
    np.testing.assert_array_equal(HipInverseTargetTransform(xform_source("scaled"))(s, d), XFORMS["scaled"][1](s, d))
    fwd = HipTargetTransform("__device__ void bbmpc_user_transform_targets(const float* cur, const float* next, float* t, "
                             "int S) { for (int i = 0; i < S; ++i) t[i] = 2.0f * (next[i] - cur[i]); }")
    np.testing.assert_array_equal(fwd(s, d), (F(2.0) * (d - s).astype(F)).astype(F))


def test_training_with_a_hip_target_transform(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.utils.device_functions import HipTargetTransform
    src = ("__device__ void bbmpc_user_transform_targets(const float* cur, const float* next, float* t, int S) {\n"
           "    for (int i = 0; i < S; ++i) t[i] = 10.0f * (next[i] - cur[i]);\n}\n")
    numpy_tf = lambda s, n: (F(10.0) * (n - s).astype(F)).astype(F)
    rng = np.random.default_rng(2)
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
    obs_l, acs_l = [], []
    for e in range(3):
        s = O.pendulum_start_states(2, agent_offset=2 * e)
        obs, acs = [s], []
        for t in range(30):
            a = rng.uniform(-2, 2, (2, 1)).astype(F)
            s = ev.predict_next_state(s, a)
            obs.append(s)
            acs.append(a)
        obs_l.append(np.array(obs))
        acs_l.append(np.array(acs))
    rews = [np.zeros((30, 2), F)] * 3
    hip_tf = HipTargetTransform(src)
    np.testing.assert_array_equal(hip_tf(obs_l[0][:-1, 0], obs_l[0][1:, 0]), numpy_tf(obs_l[0][:-1, 0], obs_l[0][1:, 0]))
    fn = DeterministicMLP([4, 16, 16, 3], ["tanh", "relu", None], seed=3)
    h = SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn,
                              transform_targets_func=hip_tf)
    w0, b0 = [w.copy() for w in fn.weights], [b.copy() for b in fn.biases]
    d_in, _ = OT.assemble_dataset(obs_l, acs_l)
    d_out = np.concatenate([numpy_tf(o[:-1, a], o[1:, a]) for o in obs_l for a in range(2)], axis=0)
    mask = rng.random(d_in.shape[0]) > 0.25
    epochs, B = 4, 32
    perms = [rng.permutation(int(mask.sum())) for _ in range(epochs)]
    h.train(obs_l, acs_l, rews, batch_size=B, learning_rate=2e-3, epochs=epochs, device="cpu", split_mask=mask,
            permutations=perms)
    np.testing.assert_array_equal(h._model_training_out, d_out[mask])
    tin, tout, vin, vout = d_in[mask], d_out[mask], d_in[~mask], d_out[~mask]
    stats = OT.normalization_stats(tin, tout, 3)
    (tin, tout), (vin, vout) = OT.normalize(tin, tout, stats, 3), OT.normalize(vin, vout, stats, 3)
    w, b, tl, vl = OT.train(w0, b0, ["tanh", "relu", None], tin, tout, vin, vout, perms, batch_size=B, learning_rate=2e-3)
    for got, want in zip(fn.weights + fn.biases, w + b):
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-4)


def test_a_transform_that_yields_nan_scores_minus_1e6(L, form):
    from blackbox_mpc_amd.engine import Engine
    eng, spec = _engine(L, "cheetah", L.REW_CHEETAH, None, 2, 5, True)
    eng.set_inverse_transform_source(
        "__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {\n"
        "    for (int i = 0; i < S; ++i) next[i] = cur[i] + dev[i];\n"
        "    if (cur[0] > 1.0e30f || dev[0] > -1.0e30f) next[17] = __int_as_float(0x7fc00000);\n}\n")
    seq = np.random.default_rng(1).uniform(-1, 1, (40, 2, 5, 6)).astype(F)
    got = eng.evaluate(_start(20, 2), seq)
    np.testing.assert_array_equal(got, np.full_like(got, -1.0e6))
    assert isinstance(Engine, type)


def test_transforms_are_refused_where_they_cannot_run(L):
    from blackbox_mpc_amd.engine import Engine
    pend = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=2)
    with pytest.raises(L.BBMPCError, match="inverse target transform"):
        pend.set_inverse_transform_source(xform_source("absolute"))
    from blackbox_mpc_amd.utils.device_functions import HipInverseTargetTransform
    from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.spaces import Box
    h = SystemDynamicsHandler(Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8]), dynamics_function=PendulumTrueModel(),
                              true_model=True, inverse_transform_targets_func=HipInverseTargetTransform(xform_source("absolute")))
    with pytest.raises(NotImplementedError, match="inverse_transform_targets_func"):
        DeterministicTrajectoryEvaluator(pendulum_reward_function, h)(O.pendulum_start_states(1), np.zeros((4, 1, 2, 1), F))
