"""CVaR scoring and quantile bands of the particle evaluator without a GPU: the NumPy statements of tests/risk_util.py
against independent ones, the alpha -> tail count and level -> rank maps, the evaluator's argument checks and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import particle_util as PU
from tests import risk_util as RU

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _returns(seed, N=41, P=7, A=3, scale=300.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, P, A)) * scale - scale).astype(F)


# ---- restatements ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 7, 64])
def test_full_tail_is_the_mean_and_one_particle_is_the_minimum(P):
    r = _returns(P, P=P)
    np.testing.assert_array_equal(RU.cvar32(r, P), PU.aggregate32(r, 0.0))
    np.testing.assert_array_equal(RU.cvar32(r, 1), r.min(axis=1))


def test_designed_ties_are_selected_by_index():
    # all equal: every k gives the value (k * v / k is exact for these k)
    r = np.full((3, 4, 2), F(-12.5))
    for k in (1, 2, 3, 4):
        np.testing.assert_array_equal(RU.cvar32(r, k), np.full((3, 2), F(-12.5)))
    np.testing.assert_array_equal(RU.stable_rank(r, 1)[0, :, 0], [0, 1, 2, 3])
    # two equal values at the cut: ranks of [5, 1, 3, 3, 0] are [4, 1, 2, 3, 0]; k = 3 takes 0, 1 and the FIRST 3
    x = np.array([5, 1, 3, 3, 0], F)
    np.testing.assert_array_equal(RU.stable_rank(x, 0), [4, 1, 2, 3, 0])
    marked = np.array([5, 1, 3, np.nextafter(F(3), F(4)), 0], F)          # the second of the pair made tellable
    assert RU.cvar32(marked.reshape(1, 5, 1), 3)[0, 0] == F((F(1) + F(3)) + F(0)) / F(3)
    swapped = marked[[0, 1, 3, 2, 4]]
    assert RU.cvar32(swapped.reshape(1, 5, 1), 3)[0, 0] == RU.cvar32(marked.reshape(1, 5, 1), 3)[0, 0]
    # k between the two equal values: exactly one of them is in, and it is the one with the lower index
    sel = RU.stable_rank(x, 0) < 3
    np.testing.assert_array_equal(sel, [False, True, True, False, True])


@pytest.mark.parametrize("P", [1, 5, 64])
def test_stable_rank_is_a_permutation_and_the_stable_argsort(P):
    rng = np.random.default_rng(P)
    x = rng.integers(0, 4, (17, P, 3)).astype(F)                # many ties
    rank = RU.stable_rank(x, 1)
    np.testing.assert_array_equal(np.sort(rank, axis=1), np.broadcast_to(np.arange(P)[None, :, None], x.shape))
    order = np.argsort(x, axis=1, kind="stable")                # order[i] = index of the value of rank i
    want = np.empty_like(order)
    np.put_along_axis(want, order, np.broadcast_to(np.arange(P)[None, :, None], x.shape).copy(), axis=1)
    np.testing.assert_array_equal(rank, want)


@pytest.mark.parametrize("P", [1, 4, 7, 64])
def test_nearest_rank_is_the_sorted_value_and_an_element(P):
    rng = np.random.default_rng(100 + P)
    x = rng.standard_normal((3, P, 5, 2)).astype(F)
    x[0, :, 0, 0] = x[0, 0, 0, 0]                               # a tied element
    ranks = sorted({0, P // 2, P - 1})
    q = RU.nearest_rank(x, ranks, 1)
    assert q.shape == (3, len(ranks), 5, 2) and q.dtype == x.dtype
    np.testing.assert_array_equal(q, np.sort(x, axis=1)[:, ranks])
    assert np.all((q[:, :, None] == x[:, None]).any(axis=2))
    np.testing.assert_array_equal(RU.nearest_rank(x, [0], 1)[:, 0], x.min(axis=1))
    np.testing.assert_array_equal(RU.nearest_rank(x, [P - 1], 1)[:, 0], x.max(axis=1))


@pytest.mark.parametrize("P,k", [(5, 1), (5, 2), (20, 4), (64, 13), (64, 64)])
def test_cvar32_is_within_the_sum_bound_of_float64(P, k):
    """aggregate_bound's kappa = 0 bound, 64 P 2^-24 max_p |r_p|, on every row: a k <= P term sum carries at most P
    ulp-level errors of a running sum no larger than k max|r|, and the division one more."""
    r = _returns(7 * P + k, N=200, P=P)
    err = np.abs(RU.cvar32(r, k).astype(np.float64) - RU.cvar64(r, k))
    bound = 64.0 * P * 2.0 ** -24 * np.abs(r.astype(np.float64)).max(axis=1)
    print("[cvar32 P=%d k=%d] max err / bound = %.3e" % (P, k, (err / bound).max()))
    assert np.all(err <= bound)


# ---- the maps -------------------------------------------------------------------------------------------------------
def test_alpha_to_tail_count_and_level_to_rank():
    from blackbox_mpc_amd.trajectory_evaluators.particle import cvar_tail_count, quantile_rank
    assert cvar_tail_count(0.1, 10) == 1                        # 0.1 * 10 = 1.0000000000000002 in floats
    assert cvar_tail_count(1.0, 10) == 10 and cvar_tail_count(1, 64) == 64
    assert cvar_tail_count(0.2, 20) == 4 and cvar_tail_count(0.21, 20) == 5 and cvar_tail_count(1e-6, 20) == 1
    assert cvar_tail_count(0.5, 1) == 1 and cvar_tail_count(0.3, 10) == 3 and cvar_tail_count(0.7, 10) == 7
    for p in (1, 3, 10, 20, 64):
        for k in range(1, p + 1):
            assert cvar_tail_count(k / p, p) == k
            assert quantile_rank(k / p, p) == k - 1
    assert quantile_rank(1.0, 20) == 19 and quantile_rank(0.05, 20) == 0 and quantile_rank(0.95, 20) == 18
    assert quantile_rank(0.5, 7) == 3 and quantile_rank(1e-9, 7) == 0 and quantile_rank(0.7, 1) == 0
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            cvar_tail_count(bad, 10)
        with pytest.raises(ValueError):
            quantile_rank(bad, 10)


def test_evaluator_argument_checks():
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.trajectory_evaluators import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    handler = SystemDynamicsHandler(Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8]), dynamics_function=PendulumTrueModel(), true_model=True)

    def make(**kw):
        return ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=10, process_noise_std=0.1, **kw)
    ev = make(risk_alpha=0.1)
    assert ev.risk_settings == (L.RISK_CVAR, 1) and len(ev.particle_settings) == 3
    assert make(risk_alpha=1.0).risk_settings == (L.RISK_CVAR, 10)
    assert make(risk_kappa=1.5).risk_settings == (L.RISK_MEAN_STD, 0) and make().risk_settings == (L.RISK_MEAN_STD, 0)
    assert make(risk_alpha=0.5, risk_kappa=0.0).risk_settings == (L.RISK_CVAR, 5)
    for bad in (dict(risk_alpha=0.2, risk_kappa=1.0), dict(risk_alpha=0.0), dict(risk_alpha=1.5), dict(risk_alpha=-0.2),
                dict(risk_alpha=float("nan")), dict(risk_alpha=float("inf"))):
        with pytest.raises(ValueError):
            make(**bad)
    assert ev.quantile_ranks([0.05, 0.5, 0.95, 1.0]) == [0, 4, 9, 9]
    for bad in ([0.0], [0.5, 1.2], [float("nan")], [], [0.1] * 9):
        with pytest.raises(ValueError):
            ev.quantile_ranks(bad)


# ---- ABI ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["bbmpc_set_particle_risk", "bbmpc_predict_trajectory_quantiles", "bbmpc_predict_trajectory_quantiles_dev"]


def test_library_exports_and_header_declares_the_entry_points(built_lib):
    lib = ctypes.CDLL(built_lib)
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)
    assert re.search(r"#define\s+BBMPC_RISK_MEAN_STD\s+0\b", text) and re.search(r"#define\s+BBMPC_RISK_CVAR\s+1\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bbmpc_[a-z_0-9]+)\s*\(", code))
    from blackbox_mpc_amd import _lib
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libbbmpc.so does not export %s" % name
        assert name in declared and name in _lib.SYMBOLS
    assert (_lib.RISK_MEAN_STD, _lib.RISK_CVAR, _lib.MAX_QUANTILE_LEVELS) == (0, 1, 8)
    # a null handle is refused by the entry points themselves, without a device
    assert lib.bbmpc_set_particle_risk(None, 1, 1) == _lib.E_INVALID
