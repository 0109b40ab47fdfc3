"""Learned terminal values without a GPU: the C header and the ctypes binding, the n-step targets on hand-computed numbers,
the LearnedValueMLP container against the float64 statement (tests/terminal_value_util.py), its trainer, and the particle
evaluator's refusal."""
import os
import re

import numpy as np
import pytest

from tests import terminal_value_util as V

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points_and_the_binding_lists_them():
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)
    for name in ("bbmpc_set_terminal_value_mlp", "bbmpc_evaluate_terminal_value", "bbmpc_evaluate_terminal_value_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    from blackbox_mpc_amd import _lib as L
    assert L.ABI_VERSION == 4
    for name in ("bbmpc_set_terminal_value_mlp", "bbmpc_evaluate_terminal_value", "bbmpc_evaluate_terminal_value_dev"):
        assert name in L.SYMBOLS
    from blackbox_mpc_amd.engine import Engine
    assert callable(Engine.set_terminal_value_mlp) and callable(Engine.evaluate_terminal_value)


def test_statement_on_hand_computed_values():
    net = V.R.Net("hand", 2, 1, 1, [2], ["relu", None], True, 0)
    net.ws = [np.array([[1.0, -1.0], [0.5, 2.0]], F), np.array([[2.0], [-1.0]], F)]
    net.bs = [np.array([0.0, 1.0], F), np.array([0.5], F)]
    net.stats = [np.array([1.0, -1.0], F), np.array([2.0, 0.5], F), np.array([10.0], F), np.array([3.0], F)]
    # s = (3, 0): x = ((3-1)/2, (0+1)/0.5) = (1, 2); layer 0 = (1 + 1, -1 + 4 + 1) = (2, 4); layer 1 = 4 - 4 + 0.5 = 0.5; V = 11.5
    np.testing.assert_allclose(V.value(net, [[3.0, 0.0]]), [11.5], rtol=0, atol=1e-5)
    base = np.array([[1.0, -1.0e6]])
    s_last = np.array([[[3.0, 0.0], [3.0, 0.0]]])
    np.testing.assert_allclose(V.with_terminal(base, net, -0.5, s_last), [[1.0 - 5.75, -1.0e6 - 5.75]], rtol=0, atol=1e-4)
    s_nan = s_last.copy()
    s_nan[0, 1, 0] = np.nan                                        # w * V is NaN: the score is -1e6, whatever the base was
    np.testing.assert_array_equal(V.with_terminal(np.array([[1.0, 7.0]]), net, 1.0, s_nan)[0, 1], -1.0e6)


def _episode():
    T, A = 5, 2
    obs = (np.arange((T + 1) * A * 3).reshape(T + 1, A, 3) * 0.5).astype(F)
    rews = np.array([[1.0, -1.0], [2.0, 0.5], [-3.0, 4.0], [0.25, 8.0], [5.0, -2.0]], F)
    return obs, rews


@pytest.mark.parametrize("gamma", [1.0, 0.9])
def test_value_targets_on_hand_computed_numbers(gamma):
    from blackbox_mpc_amd.value_functions import value_targets
    obs, rews = _episode()
    g = gamma
    # n_step = 1: every step is its own target
    s, y = value_targets(obs, rews, 1, gamma)
    np.testing.assert_array_equal(s, obs[:5].reshape(10, 3))
    np.testing.assert_allclose(y, rews.reshape(10), rtol=1e-6)
    # n_step = 3: t = 0, 1, 2; written out per agent
    s, y = value_targets(obs, rews, 3, gamma)
    want = np.array([[1.0 + g * 2.0 + g * g * -3.0, -1.0 + g * 0.5 + g * g * 4.0],
                     [2.0 + g * -3.0 + g * g * 0.25, 0.5 + g * 4.0 + g * g * 8.0],
                     [-3.0 + g * 0.25 + g * g * 5.0, 4.0 + g * 8.0 + g * g * -2.0]])
    np.testing.assert_array_equal(s, obs[:3].reshape(6, 3))
    np.testing.assert_allclose(y, want.reshape(6), rtol=1e-6)
    # n_step = 5 = T: one window per agent
    s, y = value_targets(obs, rews, 5, gamma)
    want5 = [sum(g ** k * float(rews[k, a]) for k in range(5)) for a in range(2)]
    np.testing.assert_array_equal(s, obs[0])
    np.testing.assert_allclose(y, want5, rtol=1e-6)
    # a bootstrap callable closes every window with gamma^n * f(s_{t+n})
    boot = lambda states: states[:, 0] * 2.0 + 1.0
    s, y = value_targets(obs, rews, 3, gamma, bootstrap=boot)
    tail = (obs[3:6, :, 0].astype(np.float64) * 2.0 + 1.0) * g ** 3
    np.testing.assert_allclose(y, (want + tail).reshape(6), rtol=1e-6)
    s, y = value_targets(obs, rews, 5, gamma, bootstrap=boot)
    np.testing.assert_allclose(y, np.array(want5) + g ** 5 * (obs[5, :, 0] * 2.0 + 1.0), rtol=1e-6)
    # full windows only
    s, y = value_targets(obs, rews, 6, gamma, bootstrap=boot)
    assert s.shape == (0, 3) and y.shape == (0,)


def test_container_call_statistics_save_load(tmp_path):
    from blackbox_mpc_amd.value_functions import LearnedValueMLP
    with pytest.raises(ValueError):
        LearnedValueMLP(3, [20, 2], ["tanh", None])
    rng = np.random.default_rng(4)
    for net in V.small_nets():
        m = LearnedValueMLP(net.S, net.dims[1:], net.acts)
        assert m.activation_codes == net.codes() and m.normalization_stats() is None
        v0 = m._version
        m.set_weights(net.ws, net.bs)
        m.set_normalization_stats(net.stats)
        assert m._version > v0
        states = rng.normal(0, 0.7, (19, net.S))
        want = V.value(net, states)
        got = m(states)
        assert got.dtype == np.float32 and np.all(np.abs(got - want) <= 1e-6 * np.maximum(1.0, np.abs(want)))
        path = str(tmp_path / (net.name + ".npz"))
        m.save(path)
        m2 = LearnedValueMLP.load(path)
        assert m2.layer_sizes == m.layer_sizes and m2.activation_codes == m.activation_codes
        for a, b in zip(m.weights + m.biases, m2.weights + m2.biases):
            np.testing.assert_array_equal(a, b)
        assert (m2.normalization_stats() is None) == (net.stats is None)
        if net.stats is not None:
            for a, b in zip(m.normalization_stats(), m2.normalization_stats()):
                np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(m2(states), got)


def test_train_lowers_the_loss_on_a_known_quadratic():
    from blackbox_mpc_amd.value_functions import LearnedValueMLP
    rng = np.random.default_rng(0)
    s = rng.uniform(-1, 1, (512, 3)).astype(F)
    y = 2.0 * s[:, 0] ** 2 - s[:, 1] * s[:, 2] + 0.5 * s[:, 2]
    m = LearnedValueMLP(3, [32, 1], ["tanh", None], seed=0)
    v0 = m._version
    train, val = m.train(s, y, epochs=30, batch_size=64, learning_rate=5e-3, device="cpu", seed=0)
    assert m._version > v0 and m.normalization_stats() is not None
    assert train[-1] < 0.5 * train[0] and val[-1] < val[0]
    assert np.mean((m(s) - y) ** 2) < 0.5 * np.var(y)
    # fitted n-step TD on rollouts: the targets use the model's own current prediction as the bootstrap
    obs, rews = _episode()
    m2 = LearnedValueMLP(3, [8, 1], ["tanh", None], seed=1)
    m2.train_on_rollouts([obs, obs], [rews, rews], 3, gamma=0.9, bootstrap=True, epochs=2, batch_size=4, device="cpu", seed=0)
    assert len(m2._episodes) == 2 and m2._version > 0
    with pytest.raises(ValueError, match="n_step"):
        LearnedValueMLP(3, [8, 1], ["tanh", None]).train_on_rollouts([obs], [rews], 6)


def test_particle_evaluator_refuses_a_terminal_value():
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.trajectory_evaluators.particle import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    from blackbox_mpc_amd.value_functions import LearnedValueMLP
    act_space, obs_space = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=DeterministicMLP(layers=[4, 16, 3], activation_functions=["tanh", None], seed=0))
    with pytest.raises(NotImplementedError, match="terminal"):
        ParticleTrajectoryEvaluator(pendulum_reward_function, handler, 4, 0.01, terminal_value=LearnedValueMLP(3, [8, 1], ["tanh", None]))
