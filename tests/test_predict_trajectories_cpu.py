"""What of the trajectory-prediction feature can be checked without a GPU: the header declares the new entry points, the
ctypes layer binds them, the ABI number did not move, and the window cutting of SystemDynamicsHandler.multistep_error (a
pure NumPy helper) agrees with a brute-force loop -- episodes shorter than the horizon included; hiprtc cross-compiles the run-time
compiled trajectory kernel (csrc/rtc.hpp, bbmpc_user_traj) for gfx950 with and without runtime parameters."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "bbmpc.h")).read()


def test_header_declares_the_prototypes_and_keeps_the_abi_number():
    h = re.sub(r"\s+", " ", _header())
    assert "#define BBMPC_ABI_VERSION 4" in h
    assert ("int bbmpc_predict_trajectories(bbmpc_handle h, const float* states, const float* action_sequences, int32_t batch, "
            "int32_t horizon, float* states_out, float* rewards_out);") in h
    assert ("int bbmpc_predict_trajectories_dev(bbmpc_handle h, const float* d_states, const float* d_action_sequences, "
            "int32_t batch, int32_t horizon, float* d_states_out, float* d_rewards_out);") in h
    assert "int bbmpc_trajectory_sq_error_dev(" in h


def test_lib_binds_the_symbols():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.ABI_VERSION == 4 and _lib.lib.bbmpc_abi_version() == 4
    for name, nargs in (("bbmpc_predict_trajectories", 7), ("bbmpc_predict_trajectories_dev", 7), ("bbmpc_trajectory_sq_error_dev", 6),
                        ("bbmpc_set_keep_plan", 2), ("bbmpc_get_plan", 2)):
        assert name in _lib.SYMBOLS
        fn = getattr(_lib.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    from blackbox_mpc_amd.optimizers.optimizer_base import OptimizerBase
    from blackbox_mpc_amd.policies import MPCPolicy
    assert callable(OptimizerBase.plan) and callable(MPCPolicy.plan) and callable(MPCPolicy.keep_plan)
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    assert callable(Engine.predict_trajectories) and callable(Engine.predict_trajectories_dev)
    assert callable(DeterministicTrajectoryEvaluator.predict_trajectories)


def _brute(obs_all, act_all, horizon, stride):
    starts, acts, obs_w = [], [], []
    for obs, acs in zip(obs_all, act_all):
        steps, agents = acs.shape[0], acs.shape[1]
        for agent in range(agents):
            t0 = 0
            while t0 < steps:
                if t0 + horizon <= steps:
                    starts.append(obs[t0, agent])
                    acts.append([acs[t0 + j, agent] for j in range(horizon)])
                    obs_w.append([obs[t0 + j + 1, agent] for j in range(horizon)])
                t0 += stride
    return np.array(starts, F), np.array(acts, F), np.array(obs_w, F)


@pytest.mark.parametrize("horizon,stride", [(1, 1), (5, 1), (5, 3), (12, 4), (20, 7)])
def test_window_cutting_against_a_brute_force_loop(horizon, stride):
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import multistep_windows
    rng = np.random.default_rng(horizon * 10 + stride)
    S, U, A = 4, 2, 3
    lengths = [20, 3, 12, 5, 33]                                     # some shorter than the horizon: they give no window
    obs_all = [rng.standard_normal((n + 1, A, S)).astype(F) for n in lengths]
    act_all = [rng.standard_normal((n, A, U)).astype(F) for n in lengths]
    got = multistep_windows(obs_all, act_all, horizon, stride)
    want = _brute(obs_all, act_all, horizon, stride)
    assert got[0].shape[0] == sum(A * len(range(0, n - horizon + 1, stride)) for n in lengths if n >= horizon)
    for g, w in zip(got, want):
        assert g.dtype == F and g.flags["C_CONTIGUOUS"]
        assert np.array_equal(g, w)


def test_window_cutting_with_no_window_and_bad_arguments():
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import multistep_windows
    obs, acts = [np.zeros((4, 2, 3), F)], [np.zeros((3, 2, 1), F)]
    s, a, o = multistep_windows(obs, acts, 10)
    assert s.shape == (0, 3) and a.shape == (0, 10, 1) and o.shape == (0, 10, 3)
    with pytest.raises(ValueError):
        multistep_windows(obs, acts, 0)
    with pytest.raises(ValueError):
        multistep_windows(obs, acts, 2, stride=0)
    with pytest.raises(ValueError):
        multistep_windows([np.zeros((3, 2, 3), F)], acts, 2)


def test_learning_utilities_accept_multistep_horizon():
    import inspect
    from blackbox_mpc_amd.utils.dynamics_learning import learn_dynamics_from_policy
    from blackbox_mpc_amd.utils.iterative_mpc import learn_dynamics_iteratively_w_mpc
    for fn in (learn_dynamics_from_policy, learn_dynamics_iteratively_w_mpc):
        assert inspect.signature(fn).parameters["multistep_horizon"].default is None


DYN = "__device__ void bbmpc_user_dynamics(const float* x, float* d, int S, int U) { for (int i = 0; i < S; ++i) d[i] = 0.1f * x[S + i % U] - 0.01f * x[i]; }\n"
DYN_P = ("__device__ void bbmpc_user_dynamics_params(const float* x, float* d, int S, int U, const float* params, int t) "
         "{ for (int i = 0; i < S; ++i) d[i] = params[0] * x[S + i % U] - params[1] * x[i]; }\n")
REW = "__device__ float bbmpc_user_reward(const float* c, const float* a, const float* n, int S, int U) { return -n[0] * n[0] - a[0] * a[0]; }\n"
REW_P = ("__device__ float bbmpc_user_reward_params(const float* c, const float* a, const float* n, int S, int U, const float* params, int t) "
         "{ const float d = n[0] - params[t]; return -d * d; }\n")


def test_hiprtc_cross_compiles_the_trajectory_kernel_text():
    """bbmpc_check_user_rollout / bbmpc_check_user_params compile the trajectory kernel next to the rollout (no GPU needed):
    classic and parameterised sides, user and built-in partners; a broken source is refused with the compiler's log"""
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib as L
    S, U = 5, 2
    assert L.lib.bbmpc_check_user_rollout(L.DYN_USER, L.REW_USER, DYN.encode(), REW.encode(), S, U) == 0, L.lib.bbmpc_last_error()
    assert L.lib.bbmpc_check_user_rollout(L.DYN_PENDULUM, L.REW_USER, None, REW.encode(), 3, 1) == 0, L.lib.bbmpc_last_error()
    assert L.lib.bbmpc_check_user_rollout(L.DYN_USER, L.REW_PENDULUM, DYN.encode(), None, S, U) == 0, L.lib.bbmpc_last_error()
    assert L.lib.bbmpc_check_user_params(REW_P.encode(), 40, DYN_P.encode(), 2, S, U) == 0, L.lib.bbmpc_last_error()
    assert L.lib.bbmpc_check_user_params(REW_P.encode(), 40, None, 0, S, U) == 0, L.lib.bbmpc_last_error()
    assert L.lib.bbmpc_check_user_params(None, 0, DYN_P.encode(), 2, S, U) == 0, L.lib.bbmpc_last_error()
    # the text itself is in the library and names the kernel the engine loads
    blob = open(L.LIB_PATH, "rb").read()
    assert b"bbmpc_user_traj" in blob and b"rew_rows_per_agent" in blob
    bad = REW.replace("return", "retrun")
    assert L.lib.bbmpc_check_user_rollout(L.DYN_USER, L.REW_USER, DYN.encode(), bad.encode(), S, U) == L.E_INVALID
