"""The chance constraint of the particle evaluator without a GPU: the statement of tests/chance_constraint_util.py on
hand-computed cases, StateBoxConstraint's validation, the Python refusals, the header and the binding, and the
precondition of the GPU suite's random-network cases (tests/chance_constraint_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import chance_constraint_cases as CASES
from tests import chance_constraint_util as CC

F = np.float32
INF, NAN = np.inf, np.nan
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the statement ----------------------------------------------------------------------------------------------------
def _traj(rows):
    """rows: per particle the H values of a one-feature state -> [H, N=1, P, A=1, S=1]"""
    return np.array(rows, np.float64).T[:, None, :, None, None]


def test_first_is_the_smallest_step_and_zero_means_never():
    traj = _traj([[0.0, 2.0, 0.0, 3.0],        # leaves at t = 2 and again at t = 4
                  [0.0, 0.0, 0.0, 0.0],        # never
                  [0.5, 0.9, 1.0, 1.5],        # only at t = H (1.0 is ON the bound: inside)
                  [9.0, 0.0, 0.0, 0.0]])       # at t = 1
    first = CC.first_steps(traj, [-1.0], [1.0])
    np.testing.assert_array_equal(first[0, :, 0], [2, 0, 4, 1])
    assert first.dtype == np.int32
    np.testing.assert_array_equal(CC.first_steps(traj, [-INF], [INF]), 0)           # the all-infinite box
    np.testing.assert_array_equal(CC.first_steps(-traj, [-1.0], [INF])[0, :, 0], [2, 0, 4, 1])   # a box open on one side


def test_a_nan_state_violates_nothing():
    traj = _traj([[NAN, NAN, NAN], [NAN, 5.0, NAN], [0.0, NAN, 0.0]])
    np.testing.assert_array_equal(CC.first_steps(traj, [-1.0], [1.0])[0, :, 0], [0, 2, 0])
    two = np.array([[NAN, 0.0], [NAN, 7.0], [0.0, NAN]])                              # two features: the finite one decides
    np.testing.assert_array_equal(CC.outside(two, [-1.0, -1.0], [1.0, 1.0]), [False, True, False])


def test_penalty_delta_reached_count_p_and_order_of_operations():
    first = np.array([[[1], [0], [0], [3]],     # count 2 of 4: v = 0.5
                      [[1], [2], [3], [4]],     # count = P: v = 1
                      [[0], [0], [0], [0]],     # v = 0
                      [[0], [0], [5], [0]]], np.int32)           # v = 0.25
    v = CC.violation(first)
    assert v.dtype == F
    np.testing.assert_array_equal(v[:, 0], F([0.5, 1.0, 0.0, 0.25]))
    score = F([[10.0], [10.0], [10.0], [10.0]])
    got = CC.penalised(score, v, 0.25, 8.0)
    assert got.dtype == F
    np.testing.assert_array_equal(got[:, 0], F([8.0, 4.0, 10.0, 10.0]))              # v == delta: no penalty
    np.testing.assert_array_equal(CC.penalised(score, v, 0.25, 0.0), score)          # lambda = 0
    # float32, in this order: v - delta is rounded before it is scaled
    third = CC.violation(np.array([[[1], [0], [0]]], np.int32))                      # float32(1) / float32(3)
    assert third[0, 0] == F(1.0) / F(3.0)
    want = F(1.0) - F(F(1e3) * F(F(third[0, 0]) - F(0.1)))
    assert CC.penalised(F([[1.0]]), third, 0.1, 1e3)[0, 0] == want


def test_trajectory_layouts():
    N, P, A, H, S = 3, 4, 2, 2, 1
    rows = np.arange(N * P * A, dtype=np.float64)[:, None]               # row b = (n * P + p) * A + a
    visited = [rows * 0, rows, rows + 100]
    traj = CC.trajectories(visited, N, P, A)
    assert traj.shape == (H, N, P, A, S)
    assert traj[0, 2, 3, 1, 0] == (2 * P + 3) * A + 1 and traj[1, 1, 0, 0, 0] == 100 + P * A
    half = np.arange(N * 2 * A, dtype=np.float64)[:, None]
    both = CC.member_trajectories([[half * 0, half], [half * 0, half + 1000]], N, P, A)
    assert both[0, 1, 2, 1, 0] == (1 * 2 + 1) * A + 1 and both[0, 1, 3, 1, 0] == 1000 + (1 * 2 + 1) * A + 1


# ---- the precondition of the GPU suite's cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES.CASES)))
def test_the_bound_of_every_random_case_is_ten_tolerances_from_every_row(index):
    c = CASES.case(index)
    tol = CASES.state_tolerance(c["bound"])
    ext = np.nanmax(c["traj"][..., CASES.FEATURE], axis=0)
    gap = np.abs(ext - c["bound"]).min()
    print("[chance constraint case %s/%s] bound %.6f, nearest row extreme %.3e away = %.1f state tolerances; v in [%.2f, %.2f]"
          % (c["kind"], c["reward"], c["bound"], gap, gap / tol, c["v"].min(), c["v"].max()))
    assert gap >= 10.0 * tol and c["half_gap"] >= 10.0 * tol
    assert np.all(np.isfinite(c["traj"]))
    firsts = set(np.unique(c["first"]))
    assert 0 in firsts and len(firsts) >= 3                                # never, and at least two different steps
    assert (c["v"] > CASES.DELTA).any() and (c["v"] <= CASES.DELTA).any()    # penalised and free candidates


# ---- StateBoxConstraint --------------------------------------------------------------------------------------------------
def test_state_box_constraint_validates_like_the_c_call():
    from blackbox_mpc_amd.utils.constraints import StateBoxConstraint
    box = StateBoxConstraint([-INF, -1.0], [INF, 1.0], max_violation=0.1, weight=5.0)
    np.testing.assert_array_equal(box([[0.0, 2.0], [9.0, 0.0], [NAN, 0.0], [0.0, NAN], [0.0, -1.0]]), [True, False, False, False, False])
    lo, hi = box.bounds(2)
    assert lo.dtype == F and hi.dtype == F and lo[0] == -INF and hi[1] == 1.0
    with pytest.raises(ValueError, match="coordinates"):
        box.bounds(3)
    v0 = box._version
    box.set_bounds(-2.0, 2.0)
    box.weight = 7.0
    box.max_violation = 0.0
    assert box._version == v0 + 3
    assert StateBoxConstraint().bounds(2)[0][0] == -INF                       # unbounded by default
    assert StateBoxConstraint(high=1.0).max_violation == 0.0 and StateBoxConstraint(high=1.0).weight == 1e3
    for kw in (dict(low=[NAN, 0.0]), dict(high=[0.0, NAN]), dict(low=[1.0], high=[0.0]), dict(low=[0.0, 0.0], high=[1.0]),
               dict(max_violation=1.0), dict(max_violation=-0.1), dict(max_violation=NAN), dict(max_violation=INF),
               dict(weight=-1.0), dict(weight=NAN), dict(weight=INF), dict(low=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            StateBoxConstraint(**kw)


# ---- header, binding, Python refusals ------------------------------------------------------------------------------------------
def test_header_declares_both_entry_points_and_the_binding_has_their_argument_types():
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)
    assert re.search(r"\bint\s+bbmpc_set_chance_constraint\s*\(\s*bbmpc_handle\s+h,\s*const\s+float\*\s+lo,\s*const\s+float\*\s+hi,\s*"
                     r"float\s+max_violation,\s*float\s+weight\s*\)\s*;", text)
    assert re.search(r"\bint\s+bbmpc_get_constraint_violations\s*\(\s*bbmpc_handle\s+h,\s*int32_t\s+n_pop,\s*float\*\s+prob_out,\s*"
                     r"int32_t\*\s+first_step_out\s*\)\s*;", text)
    from blackbox_mpc_amd import _lib as L
    assert L.ABI_VERSION == 4
    vp, i32, f = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert "bbmpc_set_chance_constraint" in L.SYMBOLS and "bbmpc_get_constraint_violations" in L.SYMBOLS
    assert list(L.lib.bbmpc_set_chance_constraint.argtypes) == [vp, vp, vp, f, f]
    assert list(L.lib.bbmpc_get_constraint_violations.argtypes) == [vp, i32, vp, vp]
    from blackbox_mpc_amd.engine import Engine
    assert callable(Engine.set_chance_constraint) and callable(Engine.clear_chance_constraint) and callable(Engine.constraint_violations)


def _handler_and_spaces():
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    act_space, obs_space = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=DeterministicMLP(layers=[4, 16, 3], activation_functions=["tanh", None], seed=0))
    return handler, act_space, obs_space


def test_python_refusals_come_before_any_upload():
    from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.trajectory_evaluators.particle import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.constraints import StateBoxConstraint
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    handler, act_space, obs_space = _handler_and_spaces()
    box = StateBoxConstraint([-INF, -INF, -4.0], [INF, INF, 4.0], 0.1, 50.0)
    with pytest.raises(NotImplementedError, match="DeterministicTrajectoryEvaluator"):
        DeterministicTrajectoryEvaluator(pendulum_reward_function, handler, constraint=box)
    with pytest.raises(ValueError, match="StateBoxConstraint"):
        ParticleTrajectoryEvaluator(pendulum_reward_function, handler, 4, 0.01, constraint=lambda s: s[:, 0] > 0)
    with pytest.raises(ValueError, match="coordinates"):
        ParticleTrajectoryEvaluator(pendulum_reward_function, handler, 4, 0.01, constraint=StateBoxConstraint(high=[1.0, 1.0]))
    common = dict(env_action_space=act_space, env_observation_space=obs_space, optimizer_name="CEM", num_agents=1, planning_horizon=3,
                  population_size=16, num_elite=4, max_iterations=1)
    with pytest.raises(ValueError, match="ParticleTrajectoryEvaluator"):          # the evaluator MPCPolicy builds is deterministic
        MPCPolicy(reward_function=pendulum_reward_function, dynamics_handler=handler, constraint=box, **common)
    plain = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, 4, 0.01)
    with pytest.raises(ValueError, match="ParticleTrajectoryEvaluator"):          # an evaluator that does not carry it
        MPCPolicy(trajectory_evaluator=plain, constraint=box, **common)
    with pytest.raises(ValueError, match="ParticleTrajectoryEvaluator"):
        MPCPolicy(trajectory_evaluator=DeterministicTrajectoryEvaluator(pendulum_reward_function, handler), constraint=box, **common)
    with pytest.raises(ValueError, match="constraint"):
        plain.violation_probability(np.zeros((1, 3), F), np.zeros((2, 1, 3, 1), F))
    carrying = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, 4, 0.01, constraint=box)
    assert carrying._constraint is box and not carrying._engines and not plain._engines      # nothing was created, let alone uploaded
