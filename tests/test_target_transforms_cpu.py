"""Custom target transforms without a GPU: the HIP transforms compile (hiprtc needs no device), the learned-model
rollout with a transform inlined compiles, the evaluator routes a HipInverseTargetTransform and refuses a plain callable
next to a built-in model, and train() fits a model to transformed targets exactly as the NumPy oracle does
(reference dynamics_handlers/system_dynamics_handler.py:15-17, 128-161, 314)."""
import numpy as np
import pytest

from oracle import oracle_np as O
from oracle import oracle_train as OT

F = np.float32

INVERSE_DELTA = """
__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {
    for (int i = 0; i < S; ++i) next[i] = cur[i] + dev[i];
}
"""
FORWARD_DELTA = """
__device__ void bbmpc_user_transform_targets(const float* cur, const float* next, float* target, int S) {
    for (int i = 0; i < S; ++i) target[i] = next[i] - cur[i];
}
"""
USER_REWARD = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
    float r = 0.0f;
    for (int i = 0; i < S; ++i) r = r - 0.01f * nxt[i] * nxt[i];
    for (int u = 0; u < U; ++u) r = r - 0.1f * act[u] * act[u];
    return r;
}
"""


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    return _lib


@pytest.mark.parametrize("S", [3, 17, 20, 64])
@pytest.mark.parametrize("U", [1, 6])
def test_both_transform_kinds_compile_without_a_gpu(L, S, U):
    from blackbox_mpc_amd.utils import device_functions as DF
    DF.check_source(L.USER_KIND_INVERSE_TRANSFORM, INVERSE_DELTA, S, U)
    DF.check_source(L.USER_KIND_TRANSFORM, FORWARD_DELTA, S, U)


@pytest.mark.parametrize("reward", ["pendulum", "cheetah", "user"])
def test_fused_learned_model_transform_rollout_compiles(L, reward):
    from blackbox_mpc_amd.utils import device_functions as DF
    S, U = {"pendulum": (3, 1), "cheetah": (20, 6), "user": (17, 6)}[reward]
    kind = {"pendulum": L.REW_PENDULUM, "cheetah": L.REW_CHEETAH, "user": L.REW_USER}[reward]
    DF.check_transform_rollout(INVERSE_DELTA, S, U, reward_kind=kind, reward_source=USER_REWARD if reward == "user" else None)


def test_compiler_errors_carry_the_log_and_missing_entry_points_are_refused(L):
    from blackbox_mpc_amd.utils import device_functions as DF
    broken = INVERSE_DELTA.replace("cur[i] + dev[i]", "cur[i] + undeclared_name")
    with pytest.raises(L.BBMPCError, match="undeclared_name"):
        DF.check_source(L.USER_KIND_INVERSE_TRANSFORM, broken, 3, 1)
    with pytest.raises(L.BBMPCError, match="undeclared_name"):
        DF.check_transform_rollout(broken, 20, 6)
    # the source defines the forward function only: the inverse entry point is missing
    with pytest.raises(L.BBMPCError, match="bbmpc_user_inverse_transform_targets"):
        DF.check_source(L.USER_KIND_INVERSE_TRANSFORM, FORWARD_DELTA, 3, 1)
    with pytest.raises(L.BBMPCError, match="bbmpc_user_transform_targets"):
        DF.check_source(L.USER_KIND_TRANSFORM, INVERSE_DELTA, 3, 1)
    with pytest.raises(L.BBMPCError, match="bbmpc_user_reward"):
        DF.check_transform_rollout(INVERSE_DELTA, 20, 6, reward_kind=L.REW_USER, reward_source=INVERSE_DELTA)
    # the learned model's limits
    with pytest.raises(L.BBMPCError):
        DF.check_transform_rollout(INVERSE_DELTA, 65, 1)
    # the pre-existing checks keep refusing what they refused
    assert L.lib.bbmpc_check_user_rollout(L.DYN_MLP, L.REW_USER, None, USER_REWARD.encode(), 20, 6) != 0
    assert L.lib.bbmpc_check_user_source(7, INVERSE_DELTA.encode(), 3, 1) != 0


def _mlp_handler(inverse):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    fn = DeterministicMLP([4, 16, 3], ["tanh", None], seed=0)
    return SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn,
                                 is_normalized=False, inverse_transform_targets_func=inverse)


def test_routing_accepts_a_hip_transform_and_refuses_a_plain_callable(L):
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import dynamics_plugin
    from blackbox_mpc_amd.utils.device_functions import HipInverseTargetTransform
    h = _mlp_handler(HipInverseTargetTransform(INVERSE_DELTA))
    assert dynamics_plugin(h) is h._dynamics_function
    with pytest.raises(NotImplementedError, match="inverse_transform_targets_func") as ei:
        dynamics_plugin(_mlp_handler(lambda s, d: s + d))
    assert "HipInverseTargetTransform" in str(ei.value)
    with pytest.raises(ValueError):
        HipInverseTargetTransform("  ")


def _episodes(n_eps, T, A, seed):
    """pendulum episodes under random torques, generated with the hot-path oracle's true model"""
    rng = np.random.default_rng(seed)
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
    obs_l, acs_l, rew_l = [], [], []
    for e in range(n_eps):
        s = O.pendulum_start_states(A, agent_offset=e * A)
        obs, acs, rews = [s], [], []
        for t in range(T):
            a = rng.uniform(-2, 2, (A, 1)).astype(F)
            n = ev.predict_next_state(s, a)
            rews.append(ev.evaluate_next_reward(s, n, a))
            obs.append(n)
            acs.append(a)
            s = n
        obs_l.append(np.array(obs))
        acs_l.append(np.array(acs))
        rew_l.append(np.array(rews))
    return obs_l, acs_l, rew_l


def transformed_dataset(obs_l, acs_l, transform):
    """oracle_train.assemble_dataset with the targets transform(states, next_states) per episode and agent (:314)"""
    d_in, _ = OT.assemble_dataset(obs_l, acs_l)
    outs = []
    for obs in obs_l:
        for agent in range(obs.shape[1]):
            outs.append(np.asarray(transform(obs[:-1, agent].astype(F), obs[1:, agent].astype(F)), F))
    return d_in, np.concatenate(outs, axis=0)


@pytest.mark.parametrize("name,transform", [("absolute", lambda s, n: n),
                                            ("scaled_delta", lambda s, n: ((n - s) * F(10.0)).astype(F))])
@pytest.mark.parametrize("normalized", [True, False])
def test_training_on_transformed_targets_matches_the_oracle(name, transform, normalized):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    obs, acs, rews = _episodes(4, 40, 2, 2)
    fn = DeterministicMLP([4, 16, 16, 3], ["tanh", "relu", None], seed=3)
    h = SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn,
                              is_normalized=normalized, transform_targets_func=transform)
    w0, b0 = [w.copy() for w in fn.weights], [b.copy() for b in fn.biases]
    d_in, d_out = transformed_dataset(obs, acs, transform)
    if name == "absolute":
        np.testing.assert_array_equal(d_out[:40], obs[0][1:, 0])
    rng = np.random.default_rng(4)
    mask = rng.random(d_in.shape[0]) > 0.25
    epochs, B = 6, 32
    perms = [rng.permutation(int(mask.sum())) for _ in range(epochs)]
    h.train(obs, acs, rews, validation_split=0.25, batch_size=B, learning_rate=2e-3, epochs=epochs, device="cpu",
            split_mask=mask, permutations=perms)
    np.testing.assert_array_equal(h._model_training_out, d_out[mask])
    tin, tout, vin, vout = d_in[mask], d_out[mask], d_in[~mask], d_out[~mask]
    if normalized:
        stats = OT.normalization_stats(tin, tout, 3)                        # statistics of the transformed targets
        for got, want in zip(h.normalization_stats(), stats):
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
        (tin, tout), (vin, vout) = OT.normalize(tin, tout, stats, 3), OT.normalize(vin, vout, stats, 3)
    w, b, tl, vl = OT.train(w0, b0, ["tanh", "relu", None], tin, tout, vin, vout, perms, batch_size=B, learning_rate=2e-3)
    for got, want in zip(fn.weights + fn.biases, w + b):
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-4)
    np.testing.assert_allclose(h.training_loss, tl, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(h.validation_loss, vl, rtol=1e-4, atol=1e-6)


def test_a_transform_of_the_wrong_shape_is_refused():
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    obs, acs, rews = _episodes(1, 10, 1, 0)
    h = SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]),
                              dynamics_function=DeterministicMLP([4, 8, 3], ["tanh", None], seed=0),
                              transform_targets_func=lambda s, n: n[:, :2])
    with pytest.raises(ValueError, match="transform_targets_func"):
        h.train(obs, acs, rews, epochs=1, batch_size=4, device="cpu", seed=0)
