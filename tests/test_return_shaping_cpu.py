"""Discounted, termination-aware returns without a GPU: the float64 statement (tests/return_shaping_util.py) on hand-computed
numbers, StateBoxTermination, value_targets(terminated=), the C header and the ctypes binding, the Python refusals, and
ModelEnvironment's `done`."""
import os
import re

import numpy as np
import pytest

from tests import return_shaping_util as RS

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.nan, np.inf


# ---- the statement: H = 3, one state coordinate, box [-1, 1] unless said otherwise -----------------------------------------
R3 = [1.0, 2.0, 4.0]


def _one(states, gamma=1.0, c=0.0, r=R3, lo=-1.0, hi=1.0, **kw):
    R, T = RS.shaped_return(np.array([r]), np.array(states, np.float64).reshape(1, 3, 1), gamma, [lo], [hi], c, **kw)
    return float(R[0]), int(T[0])


def test_statement_on_hand_computed_values():
    assert _one([0.0, 0.5, -0.5]) == (7.0, 0)                              # never: the plain sum
    assert _one([2.0, 0.0, 0.0]) == (1.0, 1)                               # at step 1: that step's reward counts, nothing after it
    assert _one([0.0, 0.0, -3.0]) == (7.0, 3)                              # at step H
    assert _one([0.0, 1.5, 0.0], c=-5.0) == (1.0 + 2.0 - 5.0, 2)           # c != 0 is added at the terminal step
    assert _one([0.0, 0.5, 0.5], c=-5.0) == (7.0, 0)                       # ... and only there
    assert _one([0.0, 0.5, 0.5], gamma=0.5) == (1.0 + 1.0 + 1.0, 0)        # gamma = 0.5: 1 + 0.5 * 2 + 0.25 * 4
    assert _one([0.0, 1.5, 0.0], gamma=0.5, c=-4.0) == (1.0 + 1.0 - 2.0, 2)      # c carries the terminal step's discount
    assert _one([1.0, -1.0, 0.0]) == (7.0, 0)                              # on the bound is inside
    # a NaN behind the terminal step is not read: neither a reward nor a state
    assert _one([2.0, NAN, NAN], r=[1.0, NAN, INF]) == (1.0, 1)
    # a NaN before it gives -1e6, whatever follows; T still says where the box was left
    assert _one([0.0, 2.0, 0.0], r=[NAN, 2.0, 4.0]) == (-1.0e6, 2)
    assert _one([0.0, 0.0, 0.0], r=[1.0, NAN, 4.0]) == (-1.0e6, 0)
    # a NaN state does not terminate: both comparisons are false
    assert _one([NAN, 0.0, 0.0]) == (7.0, 0)
    assert _one([NAN, 2.0, 0.0]) == (3.0, 2)
    # unbounded below / above
    assert _one([-9.0, 0.0, 2.0], lo=-INF) == (7.0, 3)
    assert _one([9.0, 0.0, -2.0], lo=-INF, hi=INF) == (7.0, 0)


def test_statement_penalty_and_terminal_value():
    base = np.array([-0.25])
    # alive: the horizon closes with gamma^H * w * V; the penalty is added after the NaN rule
    assert _one([0.0, 0.0, 0.0], gamma=0.5, base=base, vterm=np.array([8.0]), w=2.0) == (3.0 - 0.25 + 0.125 * 2.0 * 8.0, 0)
    # terminated: no value term, even a NaN one
    assert _one([0.0, 0.0, 5.0], gamma=0.5, base=base, vterm=np.array([NAN]), w=2.0) == (3.0 - 0.25, 3)
    # a NaN term makes the score -1e6 with no penalty subtracted; a NaN sum stays -1e6 + base + term
    assert _one([0.0, 0.0, 0.0], base=base, vterm=np.array([NAN])) == (-1.0e6, 0)
    assert _one([0.0, 0.0, 0.0], r=[NAN, 0.0, 0.0], base=base, vterm=np.array([1.0])) == (-1.0e6 - 0.25 + 1.0, 0)
    # gamma = 1, no bounds: today's rule
    r = np.random.default_rng(0).normal(size=(5, 2, 4))
    s = np.random.default_rng(1).normal(size=(5, 2, 4, 3))
    R, T = RS.shaped_return(r, s)
    np.testing.assert_allclose(R, r.sum(-1), rtol=1e-15)
    assert not T.any()


def test_near_bound_marks_candidates_within_the_band():
    s = np.zeros((3, 2, 2))
    s[1, 1, 0] = 1.0005
    s[2, 0, 1] = -50.04
    np.testing.assert_array_equal(RS.near_bound(s, [-INF, -50.0], [1.0, INF]), [False, True, True])
    np.testing.assert_array_equal(RS.near_bound(s, [-INF, -50.1], [1.01, INF]), [False, False, False])


# ---- StateBoxTermination ------------------------------------------------------------------------------------------------------
def test_state_box_termination_validation_and_call():
    from blackbox_mpc_amd.utils.termination import StateBoxTermination
    box = StateBoxTermination([-1.0, -INF, -8.0], [1.0, INF, 8.0], terminal_reward=-5.0)
    s = np.array([[0.0, 99.0, 0.0], [0.0, 0.0, 8.5], [-1.5, 0.0, 0.0], [NAN, NAN, NAN], [1.0, 0.0, -8.0]], F)
    got = box(s)
    assert got.dtype == bool
    np.testing.assert_array_equal(got, [False, True, True, False, False])
    np.testing.assert_array_equal(got, RS.outside(s, box.low, box.high))
    assert box(s.reshape(5, 1, 3)).shape == (5, 1) and box.terminal_reward == -5.0
    lo, hi = box.bounds(3)
    assert lo.dtype == F and hi.dtype == F
    with pytest.raises(ValueError):
        box.bounds(4)
    # scalars and None broadcast
    half = StateBoxTermination(high=2.0)
    np.testing.assert_array_equal(half(np.array([[0.0, 3.0], [-1e9, 2.0]])), [True, False])
    lo, hi = half.bounds(2)
    np.testing.assert_array_equal(lo, [-INF, -INF])
    np.testing.assert_array_equal(hi, [2.0, 2.0])
    # the version counter moves with every change
    v = box._version
    box.set_bounds([-1.0, -INF, -4.0], [1.0, INF, 4.0])
    assert box._version > v and box(s[4])
    v = box._version
    box.terminal_reward = -1.0
    assert box._version > v
    for bad in (dict(low=[NAN, 0.0]), dict(low=[1.0], high=[0.0]), dict(low=[0.0, 0.0], high=[1.0, 1.0, 1.0]), dict(low=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            StateBoxTermination(**bad)
    for bad_c in (NAN, INF):
        with pytest.raises(ValueError):
            StateBoxTermination(terminal_reward=bad_c)


# ---- value_targets(terminated=) ------------------------------------------------------------------------------------------------
def _episode():
    T, A = 6, 2
    obs = (np.arange((T + 1) * A * 3).reshape(T + 1, A, 3) * 0.5).astype(F)
    rews = np.array([[1.0, -1.0], [2.0, 0.5], [-3.0, 4.0], [0.25, 8.0], [5.0, -2.0], [0.5, 1.5]], F)
    done = np.zeros((T, A), bool)
    done[2, 0] = True                                                      # agent 0: step 2 reaches a terminal state
    done[4, 1] = True
    return obs, rews, done


@pytest.mark.parametrize("gamma", [1.0, 0.9])
@pytest.mark.parametrize("n_step", [1, 3, 6])
def test_value_targets_with_terminated_against_a_loop_written_out(gamma, n_step):
    from blackbox_mpc_amd.value_functions import value_targets
    obs, rews, done = _episode()
    T, A = rews.shape
    boot = lambda states: states[:, 0].astype(np.float64) * 2.0 + 1.0
    for bootstrap in (None, boot):
        s, y = value_targets(obs, rews, n_step, gamma, bootstrap=bootstrap, terminated=done)
        M = T - n_step + 1
        want = np.zeros((M, A))
        for t in range(M):
            for a in range(A):
                tot, alive = 0.0, True
                for k in range(n_step):
                    tot += gamma ** k * float(rews[t + k, a])
                    if done[t + k, a]:
                        alive = False
                        break
                if alive and bootstrap is not None:
                    tot += gamma ** n_step * float(boot(obs[t + n_step, a][None])[0])
                want[t, a] = tot
        np.testing.assert_array_equal(s, obs[:M].reshape(M * A, 3))
        np.testing.assert_allclose(y, want.reshape(-1), rtol=1e-6)
        # None, and an all-false array, reproduce today's targets exactly
        s0, y0 = value_targets(obs, rews, n_step, gamma, bootstrap=bootstrap)
        s1, y1 = value_targets(obs, rews, n_step, gamma, bootstrap=bootstrap, terminated=None)
        s2, y2 = value_targets(obs, rews, n_step, gamma, bootstrap=bootstrap, terminated=np.zeros((T, A), bool))
        np.testing.assert_array_equal(y0, y1)
        np.testing.assert_array_equal(y0, y2)
        np.testing.assert_array_equal(s0, s2)
    s3, y3 = value_targets(obs, rews, n_step, gamma, terminated=done[:, 0])         # [T]: every agent
    assert y3.shape == y.shape
    with pytest.raises(ValueError, match="terminated"):
        value_targets(obs, rews, n_step, gamma, terminated=np.zeros((T + 1, A), bool))


def test_train_on_rollouts_passes_terminated_through():
    from blackbox_mpc_amd.value_functions import LearnedValueMLP, value_targets
    obs, rews, done = _episode()
    seen = {}
    m = LearnedValueMLP(3, [8, 1], ["tanh", None], seed=1)
    m.train = lambda states, targets, **kw: seen.update(states=states, targets=targets)
    m.train_on_rollouts([obs, obs], [rews, rews], 3, gamma=0.9, terminated=[done, None])
    y_done, y_plain = value_targets(obs, rews, 3, 0.9, terminated=done)[1], value_targets(obs, rews, 3, 0.9)[1]
    np.testing.assert_array_equal(seen["targets"], np.concatenate([y_done, y_plain]))
    assert np.max(np.abs(y_done - y_plain)) > 0.1
    with pytest.raises(ValueError, match="terminated"):
        m.train_on_rollouts([obs], [rews], 3, terminated=[done, done])


# ---- header, binding, Python refusals ------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_binding_lists_them():
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)
    for name in ("bbmpc_set_return_shaping", "bbmpc_get_termination_steps"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    from blackbox_mpc_amd import _lib as L
    assert L.ABI_VERSION == 4
    for name in ("bbmpc_set_return_shaping", "bbmpc_get_termination_steps"):
        assert name in L.SYMBOLS and hasattr(L.lib, name)
    from blackbox_mpc_amd.engine import Engine
    assert callable(Engine.set_return_shaping) and callable(Engine.termination_steps)


def _handler_and_spaces():
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    act_space, obs_space = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=DeterministicMLP(layers=[4, 16, 3], activation_functions=["tanh", None], seed=0))
    return handler, act_space, obs_space


def test_python_refusals_come_before_any_upload():
    from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.trajectory_evaluators.particle import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    from blackbox_mpc_amd.utils.termination import StateBoxTermination
    handler, act_space, obs_space = _handler_and_spaces()
    box = StateBoxTermination([-INF, -INF, -4.0], [INF, INF, 4.0], -5.0)
    for kw in (dict(termination=box), dict(discount=0.9)):
        with pytest.raises(NotImplementedError, match="discount"):
            ParticleTrajectoryEvaluator(pendulum_reward_function, handler, 4, 0.01, **kw)
    for bad in (0.0, 1.5, -0.1, NAN, INF):
        with pytest.raises(ValueError, match="discount"):
            DeterministicTrajectoryEvaluator(pendulum_reward_function, handler, discount=bad)
    with pytest.raises(ValueError, match="StateBoxTermination"):
        DeterministicTrajectoryEvaluator(pendulum_reward_function, handler, termination=lambda s: s[:, 0] > 0)
    rew = LearnedRewardMLP(3, 1, [8, 1], ["tanh", None], seed=0)
    for kw in (dict(termination=box), dict(discount=0.9)):
        ev = DeterministicTrajectoryEvaluator(rew, handler, **kw)
        with pytest.raises(ValueError, match="value_and_gradient"):
            ev.value_and_gradient(np.zeros((1, 3), F), np.zeros((2, 1, 3, 1), F))
        assert not ev._engines                                              # nothing was created, let alone uploaded
        common = dict(reward_function=rew, env_action_space=act_space, env_observation_space=obs_space, dynamics_handler=handler,
                      optimizer_name="CEM", num_agents=1, planning_horizon=3, population_size=16, num_elite=4, max_iterations=1)
        with pytest.raises(ValueError, match="refine_steps"):
            MPCPolicy(refine_steps=2, **common, **kw)
        with pytest.raises(ValueError, match="grad_steps"):
            MPCPolicy(grad_steps=2, **common, **kw)
        with pytest.raises(ValueError, match="trajectory evaluator"):
            MPCPolicy(trajectory_evaluator=ev, optimizer_name="CEM", num_agents=1, env_action_space=act_space,
                      env_observation_space=obs_space, planning_horizon=3, population_size=16, num_elite=4, max_iterations=1, **kw)


def test_model_environment_reports_done_from_the_evaluators_termination():
    from blackbox_mpc_amd.utils.rollouts import ModelEnvironment
    from blackbox_mpc_amd.utils.termination import StateBoxTermination

    class Stub:
        _system_dynamics_handler = None

        def predict_next_state(self, s, a):
            return (s + a).astype(F)

        def evaluate_next_reward(self, s, n, a):
            return np.zeros(s.shape[0], F)

    start = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 0.0]], F)
    ev = Stub()
    env = ModelEnvironment(ev, start)
    assert env.step(np.ones((3, 2), F))[2] is False                        # no termination: as it always was
    ev._termination = StateBoxTermination(high=[1.2, INF])
    env = ModelEnvironment(ev, start)
    obs, rew, done, info = env.step(np.array([[1.0, 9.0], [1.0, 0.0], [NAN, 0.0]], F))
    assert done.dtype == bool
    np.testing.assert_array_equal(done, [False, True, False])
    np.testing.assert_array_equal(env.step(np.full((3, 2), 0.5, F))[2], [True, True, False])
