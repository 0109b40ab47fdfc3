"""Runtime parameters of HIP-source reward / dynamics functions, CPU side: a parameterised source compiles into every
program it takes part in (row kernels, trajectory scorer, fused rollouts with each partner, the learned model's
transform rollout with the reward inlined) without a GPU; a declaration that does not match the entry point the source
defines fails with the missing name in the compiler log; the Python objects validate num_params and set_params."""
import numpy as np
import pytest

from blackbox_mpc_amd import _lib as L
from blackbox_mpc_amd.utils.device_functions import HipDynamicsFunction, HipRewardFunction, check_params_source

GOAL_REWARD = """
__device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,
                                          const float* params, int t) {
    float r = 0.0f;
    for (int i = 0; i < S; ++i) { const float d = nxt[i] - params[i]; r -= d * d; }
    for (int u = 0; u < U; ++u) r -= params[S] * act[u] * act[u];
    return r + 0.0f * (float)t;
}
"""
MASS_DYNAMICS = """
__device__ void bbmpc_user_dynamics_params(const float* x, float* delta, int S, int U, const float* params, int t) {
    for (int i = 0; i < S; ++i) delta[i] = 0.05f * x[S + (i % U)] / params[0] - 0.01f * x[i];
}
"""
CLASSIC_REWARD = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) { return -nxt[0]; }
"""
CLASSIC_DYNAMICS = """
__device__ void bbmpc_user_dynamics(const float* x, float* delta, int S, int U) { for (int i = 0; i < S; ++i) delta[i] = 0.0f; }
"""


def test_parameterised_functions_compile_into_every_program(built_lib):
    # the reward: rows + traj scorer, fused with the built-in pendulum model and with a user model, the learned model's
    # transform rollout; the dynamics: rows (with and without an inverse transform), fused with each built-in reward and
    # with a user reward -- parameterised on both sides at once as well
    check_params_source(3, 1, reward_source=GOAL_REWARD, reward_params=4)
    check_params_source(20, 6, reward_source=GOAL_REWARD, reward_params=21)
    check_params_source(3, 1, dynamics_source=MASS_DYNAMICS, dynamics_params=1)
    check_params_source(3, 1, reward_source=GOAL_REWARD, reward_params=4, dynamics_source=MASS_DYNAMICS, dynamics_params=1)
    check_params_source(4, 2, reward_source=GOAL_REWARD, reward_params=L.MAX_USER_PARAMS,
                        dynamics_source=MASS_DYNAMICS, dynamics_params=L.MAX_USER_PARAMS)


def test_a_declaration_that_does_not_match_the_source_names_the_missing_function(built_lib):
    with pytest.raises(L.BBMPCError) as ei:                  # declared with parameters, defines the classic entry point
        check_params_source(3, 1, reward_source=CLASSIC_REWARD, reward_params=2)
    assert ei.value.code == L.E_INVALID and "bbmpc_user_reward_params" in str(ei.value)
    with pytest.raises(L.BBMPCError) as ei:
        check_params_source(3, 1, dynamics_source=CLASSIC_DYNAMICS, dynamics_params=2)
    assert "bbmpc_user_dynamics_params" in str(ei.value)
    # the reverse: a classic declaration of a source that only defines the parameterised entry point
    with pytest.raises(L.BBMPCError) as ei:
        L.check(L.lib.bbmpc_check_user_source(L.USER_KIND_REWARD, GOAL_REWARD.encode(), 3, 1))
    assert "bbmpc_user_reward" in str(ei.value)
    with pytest.raises(L.BBMPCError) as ei:
        L.check(L.lib.bbmpc_check_user_rollout(L.DYN_USER, L.REW_PENDULUM, MASS_DYNAMICS.encode(), None, 3, 1))
    assert "bbmpc_user_dynamics" in str(ei.value)


def test_num_params_limits_at_the_abi(built_lib):
    with pytest.raises(L.BBMPCError) as ei:
        check_params_source(3, 1, reward_source=GOAL_REWARD, reward_params=L.MAX_USER_PARAMS + 1)
    assert ei.value.code == L.E_UNSUPPORTED
    with pytest.raises(L.BBMPCError) as ei:
        check_params_source(3, 1, reward_source=GOAL_REWARD, reward_params=0)
    assert ei.value.code == L.E_INVALID


def test_num_params_is_validated():
    for bad in (-1, L.MAX_USER_PARAMS + 1):
        with pytest.raises(ValueError):
            HipRewardFunction(GOAL_REWARD, num_params=bad)
        with pytest.raises(ValueError):
            HipDynamicsFunction(MASS_DYNAMICS, 3, 1, num_params=bad)
    for bad in (1.5, "3", True):
        with pytest.raises(TypeError):
            HipRewardFunction(GOAL_REWARD, num_params=bad)
    assert HipRewardFunction(GOAL_REWARD, num_params=L.MAX_USER_PARAMS).num_params == L.MAX_USER_PARAMS
    assert HipRewardFunction(CLASSIC_REWARD).num_params == 0


def test_set_params_validates_and_copies():
    f = HipRewardFunction(GOAL_REWARD, num_params=4)
    assert f._params is None and f._params_version == 0
    for bad in (np.zeros(3), np.zeros(5), np.zeros((2, 3)), np.zeros((0, 4)), np.zeros((2, 2, 4)), 1.0):
        with pytest.raises(ValueError):
            f.set_params(bad)
    assert f._params_version == 0                            # a refused call leaves the function as it was
    goal = np.array([1.0, 2.0, 3.0, 4.0])
    f.set_params(goal)
    goal[0] = 99.0                                           # the caller's array is not aliased
    assert f._params.dtype == np.float32 and f._params.tolist() == [1.0, 2.0, 3.0, 4.0] and f._params_version == 1
    f.set_params(np.arange(12).reshape(3, 4))               # per agent
    assert f._params.shape == (3, 4) and f._params_version == 2
    d = HipDynamicsFunction(MASS_DYNAMICS, 3, 1, num_params=1)
    d.set_params([2.0])
    assert d._params.shape == (1,) and d._params_version == 1


def test_set_params_on_a_classic_function_is_refused():
    with pytest.raises(ValueError):
        HipRewardFunction(CLASSIC_REWARD).set_params([1.0])
    with pytest.raises(ValueError):
        HipDynamicsFunction(CLASSIC_DYNAMICS, 3, 1).set_params([1.0])


def test_direct_calls_refuse_per_agent_parameters():
    f = HipRewardFunction(GOAL_REWARD, num_params=4)
    f.set_params(np.zeros((2, 4)))
    z = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError):                          # refused before any engine (or GPU) is touched
        f(z, np.zeros((2, 1), np.float32), z)
