"""CPU-side checks of CEM's elite carry-over: the NumPy statement of the rule, CEMOptimizer's argument
checks and the C ABI's new entry points (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import correlated_util as CU
from tests import elite_carry_util as EC

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, A, H, ITERS, K = 40, 2, 6, 3, 6


def _evaluator():
    return O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))


def _noise(seed, U=1):
    rng = np.random.default_rng(seed)
    return {"trunc": [O.truncated_normal_noise(rng, (N, A, H, U)) for _ in range(ITERS)]}


def _kw():
    return dict(horizon=H, max_iterations=ITERS, population=N, num_elite=K, num_agents=A)


def test_carry_off_is_the_oracle_bit_for_bit():
    states = O.pendulum_start_states(A)
    base = O.CEM(_evaluator(), [-2.0], [2.0], **_kw())
    own = EC.CarryCEM(_evaluator(), [-2.0], [2.0], keep=0, shift=0, **_kw())
    for step in range(2):
        noise = _noise(step)
        np.testing.assert_array_equal(own._optimize(states, noise), base._optimize(states, noise))
        for it in range(ITERS):
            for key in ("samples", "rewards", "elites", "mean", "var"):
                np.testing.assert_array_equal(own.trace[it][key], base.trace[it][key])
        assert own.stored is None
    # ... and with a matrix, correlated_util.CorrelatedCEM
    M = np.random.default_rng(3).normal(0.0, 0.8, (H, H)).astype(F)
    base = CU.CorrelatedCEM(_evaluator(), [-2.0], [2.0], mix=M, **_kw())
    own = EC.CarryCEM(_evaluator(), [-2.0], [2.0], mix=M, **_kw())
    noise = _noise(5)
    np.testing.assert_array_equal(own._optimize(states, noise), base._optimize(states, noise))
    for it in range(ITERS):
        for key in ("samples", "rewards", "elites", "mean", "var"):
            np.testing.assert_array_equal(own.trace[it][key], base.trace[it][key])


@pytest.mark.parametrize("keep", [1, 3])
@pytest.mark.parametrize("with_mix", [False, True])
def test_kept_elites_make_the_best_reward_monotone(keep, with_mix):
    M = np.random.default_rng(4).normal(0.0, 0.8, (H, H)).astype(F) if with_mix else None
    cem = EC.CarryCEM(_evaluator(), [-2.0], [2.0], keep=keep, shift=0, mix=M, **_kw())
    plain = EC.CarryCEM(_evaluator(), [-2.0], [2.0], mix=M, **_kw())
    states = O.pendulum_start_states(A)
    noise = _noise(7)
    cem._optimize(states, noise)
    plain._optimize(states, noise)
    best = np.stack([t["rewards"].max(axis=0) for t in cem.trace])            # [iters, A]
    assert np.all(np.diff(best, axis=0) >= 0.0)                               # the same rows give the same float32 rewards
    for it in range(1, ITERS):
        prev, cur = cem.trace[it - 1], cem.trace[it]
        for a in range(A):
            np.testing.assert_array_equal(cur["samples"][N - keep:, a], prev["samples"][prev["elites"][a][:keep], a])
            np.testing.assert_array_equal(cur["rewards"][N - keep:, a], prev["rewards"][prev["elites"][a][:keep], a])
    np.testing.assert_array_equal(cem.trace[0]["samples"], plain.trace[0]["samples"])     # iteration 0 has no replaced column
    assert cem.stored is None                                                 # shift = 0: nothing for the next control step


@pytest.mark.parametrize("U", [1, 2])
def test_shifted_columns_of_the_second_control_step(U):
    lo, hi = [-2.0] * U, [2.0] * U
    ev = lambda s, x: (-np.square(x - F(0.5)).sum(axis=(2, 3))).astype(F)     # noqa: E731  (any reward: the rule is about samples)
    keep, shift = 2, 3
    cem = EC.CarryCEM(ev, lo, hi, keep=keep, shift=shift, **_kw())
    plain = EC.CarryCEM(ev, lo, hi, **_kw())
    states = np.zeros((A, 3), F)
    noise = _noise(11, U)
    cem._optimize(states, noise)
    last = cem.trace[-1]
    assert cem.stored.shape == (shift, A, H, U)
    cem._optimize(states, noise)
    plain._optimize(states, noise)
    first = cem.trace[0]["samples"]
    np.testing.assert_array_equal(first[:N - shift], plain.trace[0]["samples"][:N - shift])    # Q2: same mean, same draws
    for a in range(A):
        for e in range(shift):
            row = last["samples"][last["elites"][a][e], a]                    # [H,U]
            np.testing.assert_array_equal(first[N - shift + e, a, :H - 1], row[1:])
            np.testing.assert_array_equal(first[N - shift + e, a, H - 1], row[H - 1])
    # reset() drops them
    cem.reset()
    assert cem.stored is None
    cem._optimize(states, noise)
    np.testing.assert_array_equal(cem.trace[0]["samples"], plain.trace[0]["samples"])


def _spaces():
    from blackbox_mpc_amd import Box
    return Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])


def test_cem_optimizer_argument_checks(built_lib):
    from blackbox_mpc_amd.optimizers import CEMOptimizer
    act, obs = _spaces()
    kw = dict(env_action_space=act, env_observation_space=obs, planning_horizon=6, num_agents=2, population_size=50, num_elite=8)
    assert CEMOptimizer(**kw)._elite_carry == (0, 0)
    assert CEMOptimizer(keep_elites=3, shift_elites=2, **kw)._elite_carry == (3, 2)
    assert CEMOptimizer(keep_elites=8, shift_elites=np.int64(8), **kw)._elite_carry == (8, 8)
    for name in ("keep_elites", "shift_elites"):
        for bad in (-1, 9, 1.0, 2.5, "2", None, True):
            with pytest.raises(ValueError, match=name):
                CEMOptimizer(**{name: bad}, **kw)


@pytest.mark.parametrize("name", ["PI2Optimizer", "RandomSearchOptimizer", "PSOOptimizer", "SPSAOptimizer", "CMAESOptimizer"])
def test_the_other_optimizers_do_not_take_the_arguments(built_lib, name):
    from blackbox_mpc_amd import optimizers as OPT
    act, obs = _spaces()
    for kwarg in ({"keep_elites": 1}, {"shift_elites": 1}):
        with pytest.raises(TypeError):
            getattr(OPT, name)(env_action_space=act, env_observation_space=obs, planning_horizon=5, num_agents=1, **kwarg)


def test_new_symbols_declared_and_exported(built_lib):
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bbmpc_[a-z_0-9]+)\s*\(", text))
    lib = ctypes.CDLL(built_lib)
    from blackbox_mpc_amd import _lib
    for name in ("bbmpc_set_elite_carry", "bbmpc_get_elite_carry"):
        assert name in declared and name in _lib.SYMBOLS
        assert hasattr(lib, name), "libbbmpc.so does not export %s" % name
    # a null handle is refused with BBMPC_E_INVALID before anything else
    assert _lib.lib.bbmpc_set_elite_carry(None, 1, 1) == _lib.E_INVALID
    v = [ctypes.c_int(7) for _ in range(3)]
    assert _lib.lib.bbmpc_get_elite_carry(None, *[ctypes.byref(x) for x in v]) == _lib.E_INVALID
    assert [x.value for x in v] == [7, 7, 7]
