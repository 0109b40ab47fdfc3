"""Particle trajectory evaluator without a GPU: the NumPy helper the GPU tests compare against (tests/particle_util.py)
is checked against the oracle and its own float64 twin, the C ABI's argument handling that needs no device, the Python
class's forwarding, and SystemDynamicsHandler.residual_std on the host training row."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import particle_util as PU

F = np.float32
R_RTOL, R_ATOL = 2e-4, 2e-3                 # tests/test_gpu_pendulum.py
PEND_SIGMA = np.array([0.01, 0.01, 0.05], F)
AGG_SIGMA = np.array([0.05, 0.05, 0.25], F)   # the aggregate tests': every row's returns spread by >= 1 % of their size
PEND_SHAPES = [(1, 1, 1, 1), (65, 3, 5, 7), (257, 2, 8, 20)]          # (N, A, P, H) of the GPU test


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    return _lib


def pendulum_case(N, A, P, H):
    rng = np.random.default_rng(N * 1009 + A * 101 + P * 11 + H)
    return (O.pendulum_start_states(A), rng.uniform(-2, 2, (N, A, H, 1)).astype(F),
            rng.standard_normal((A, P, H, 3)).astype(F))


def _pendulum_ev():
    return O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))


def _mlp_ev():
    ws, bs = O.make_mlp_params([4, 16, 3], seed=1)
    return O.Evaluator("pendulum", O.Handler(O.MLP(ws, bs, ["tanh", None]), False, False))


@pytest.mark.parametrize("make_ev", [_pendulum_ev, _mlp_ev])
def test_helper_is_the_oracle_evaluator_without_noise(make_ev):
    ev = make_ev()
    N, A, H = 33, 3, 9
    rng = np.random.default_rng(0)
    states = O.pendulum_start_states(A)
    seq = rng.uniform(-2, 2, (N, A, H, 1)).astype(F)
    pe = PU.ParticleEvaluator(ev.reward, ev.handler, 1, np.zeros(3, F), 0.0, rng.standard_normal((A, 1, H, 3)))
    np.testing.assert_array_equal(pe(states, seq), ev(states, seq))
    np.testing.assert_array_equal(pe.last_returns[:, 0], ev(states, seq))
    # ... and the noise is common to the candidates: two equal candidates score equally, particle by particle
    pe3 = PU.ParticleEvaluator(ev.reward, ev.handler, 3, PEND_SIGMA, 1.0, rng.standard_normal((A, 3, H, 3)))
    r = pe3.returns(states, np.concatenate([seq[:1], seq[:1]]))
    np.testing.assert_array_equal(r[0], r[1])
    assert np.all(r[0, 0] != r[0, 1])


@pytest.mark.parametrize("N,A,P,H", PEND_SHAPES)
def test_float32_helper_needs_no_excuse_against_its_float64_twin(N, A, P, H):
    """The GPU test lets at most 1 % of the device's returns miss the tolerance, and only where they are closer to the
    float64 recurrence than the float32 helper is: on these seeds the helper itself is inside the tolerance everywhere."""
    states, seq, eps = pendulum_case(N, A, P, H)
    r32 = PU.particle_returns(_pendulum_ev(), states, seq, eps, PEND_SIGMA, P)
    r64 = PU.pendulum_particle_returns64(states, seq, eps, PEND_SIGMA.astype(np.float64), P)
    assert r32.shape == (N, P, A)
    np.testing.assert_allclose(r32, r64, rtol=R_RTOL, atol=R_ATOL)


@pytest.mark.parametrize("kappa", [0.0, 1.5])
def test_helper_aggregate_against_float64(kappa):
    """The bound of the GPU test, on the helper's own returns: at most 10 % of the rows have a float64 std below 1 % of
    max |r_p| and are left out -- AGG_SIGMA is chosen so (at PEND_SIGMA nearly half of them would be)."""
    N, A, P, H = 257, 2, 8, 20
    states, seq, eps = pendulum_case(N, A, P, H)
    r = PU.particle_returns(_pendulum_ev(), states, seq, eps, AGG_SIGMA, P)
    bound, rows = PU.aggregate_bound(r, kappa)
    assert rows.mean() >= 0.9, "only %.1f %% of the rows spread enough for the bound" % (100 * rows.mean())
    err = np.abs(PU.aggregate32(r, kappa).astype(np.float64) - PU.aggregate64(r, kappa))
    assert np.all(err[rows] <= bound[rows]), (err[rows] / bound[rows]).max()
    if kappa == 0.0:                                     # the mean alone holds the bound on every row
        assert np.all(err <= bound)


def test_process_noise_statement_is_standard_normal_and_keyed():
    z = PU.process_noise_np(0x1234, 3, 1, 2, 3, 5, 3)
    assert z.shape == (2, 3, 5, 3)
    big = PU.process_noise_np(7, 0, 0, 4, 16, 50, 20).ravel()
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02
    # sharding by agents: agent 1 of a two-agent handle = agent 0 of a handle at agent_offset 1
    np.testing.assert_array_equal(PU.process_noise_np(9, 2, 1, 2, 3, 5, 3)[1], PU.process_noise_np(9, 2, 1, 1, 3, 5, 3, agent_offset=1)[0])


def test_abi_argument_codes_without_a_device(L):
    sigma = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
    assert L.lib.bbmpc_set_particles(None, 4, sigma, ctypes.c_float(0.0)) == L.E_INVALID
    assert b"null handle" in L.lib.bbmpc_last_error()
    out = (ctypes.c_float * 4)()
    assert L.lib.bbmpc_evaluate_particles(None, out, out, 1, out, None) == L.E_INVALID
    assert L.lib.bbmpc_evaluate_particles_dev(None, out, out, 1, out, None) == L.E_INVALID
    assert L.NOISE_PROCESS == 11 and L.MAX_PARTICLES == 64
    if L.device_count() == 0:                            # a missing device is reported as everywhere else
        from blackbox_mpc_amd.engine import Engine
        with pytest.raises(L.BBMPCError) as ei:
            Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=4)
        assert ei.value.code == L.E_NO_DEVICE


def test_header_declares_what_the_binding_names(L):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbmpc.h")).read()
    for sym in ("bbmpc_set_particles", "bbmpc_evaluate_particles", "bbmpc_evaluate_particles_dev"):
        assert "int %s(" % sym in header and sym in L.SYMBOLS and hasattr(L.lib, sym)
    assert "#define BBMPC_NOISE_PROCESS           11" in header


def _true_handler():
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel
    return SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]),
                                 dynamics_function=PendulumTrueModel(), true_model=True)


def test_python_class_forwards_its_arguments(L):
    from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator, ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    h = _true_handler()
    ev = ParticleTrajectoryEvaluator(pendulum_reward_function, h, num_particles=6, process_noise_std=[0.01, 0.02, 0.03],
                                     risk_kappa=1.5, quirks=L.FIX_Q1_REWARD_ARG_ORDER)
    assert isinstance(ev, DeterministicTrajectoryEvaluator)
    p, sg, kappa = ev.particle_settings
    assert p == 6 and kappa == 1.5 and sg.dtype == np.float32
    np.testing.assert_array_equal(sg, np.array([0.01, 0.02, 0.03], F))
    assert ev._quirks == L.FIX_Q1_REWARD_ARG_ORDER
    np.testing.assert_array_equal(ParticleTrajectoryEvaluator(pendulum_reward_function, h, 2, 0.5).particle_settings[1], np.full(3, 0.5, F))
    assert ParticleTrajectoryEvaluator(pendulum_reward_function, h, 2, 0.5).particle_settings[2] == 0.0
    for bad in (dict(num_particles=0, process_noise_std=0.1), dict(num_particles=65, process_noise_std=0.1),
                dict(num_particles=2, process_noise_std=-0.1), dict(num_particles=2, process_noise_std=[0.1, 0.1]),
                dict(num_particles=2, process_noise_std=np.nan), dict(num_particles=2, process_noise_std=0.1, risk_kappa=np.inf)):
        with pytest.raises(ValueError):
            ParticleTrajectoryEvaluator(pendulum_reward_function, h, **bad)

    # OptimizerBase.set_trajectory_evaluator hands the settings to the engine it builds (a recording stand-in: no GPU here)
    from blackbox_mpc_amd.optimizers import optimizer_base as OB
    calls = []

    class FakeEngine:
        _param_fns = {}

        def __init__(self, *a, **kw):
            self.cfg = type("C", (), {"dynamics": L.DYN_PENDULUM, "reward": L.REW_PENDULUM})()

        def set_particles(self, *a):
            calls.append(a)

        def close(self):
            pass

    from blackbox_mpc_amd.optimizers import RandomSearchOptimizer
    real = OB.Engine
    OB.Engine = FakeEngine
    try:
        opt = RandomSearchOptimizer(h._env_action_space, h._env_observation_space, planning_horizon=5, population_size=8, num_agents=1)
        opt.set_trajectory_evaluator(ev)
        assert len(calls) == 1 and calls[0][0] == 6 and calls[0][2] == 1.5
        np.testing.assert_array_equal(calls[0][1], sg)
        opt.set_trajectory_evaluator(DeterministicTrajectoryEvaluator(pendulum_reward_function, h))
        assert len(calls) == 1                                       # a deterministic evaluator: what it did before
    finally:
        OB.Engine = real


def test_residual_std_on_the_host_training_row():
    from tests.test_train_cpu import _episodes, _handler
    obs, acs, rews = _episodes(4, 40, 2, 2)
    for normalized in (True, False):
        h, fn = _handler(normalized=normalized, seed=3)
        with pytest.raises(Exception, match="train"):
            h.residual_std()
        rng = np.random.default_rng(4)
        mask = rng.random(4 * 2 * 40) > 0.25
        perms = [rng.permutation(int(mask.sum())) for _ in range(3)]
        h.train(obs, acs, rews, batch_size=32, learning_rate=2e-3, epochs=3, device="cpu", split_mask=mask, permutations=perms)
        got = h.residual_std()
        assert got.shape == (3,) and got.dtype == np.float32 and np.all(got > 0)
        # the same figure from the fitted model through the oracle: RMS of (target - prediction) on the validation rows
        ev = O.Evaluator("pendulum", O.Handler(O.MLP(fn.weights, fn.biases, ["tanh", "relu", None]), False, normalized,
                                               h.normalization_stats() if normalized else None))
        vin, vout = h._model_validation_in, h._model_validation_out
        pred = ev.predict_next_state(vin[:, :3], vin[:, 3:]).astype(np.float64) - vin[:, :3]
        want = np.sqrt(np.mean((vout - pred) ** 2, axis=0))
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6)
