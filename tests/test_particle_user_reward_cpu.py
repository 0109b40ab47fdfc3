"""What the particle evaluator's HIP-source rewards need without a GPU: the NumPy twins of tests/particle_user_reward_util.py
against float64 restatements, and the reward program -- now with the two particle scorers in it (csrc/rtc.hpp) --
cross-compiling for every test source, with and without runtime parameters."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import particle_user_reward_util as RU
from tests import particle_util as PU

F = np.float32


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    return _lib


def _rows(seed, B=6):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (B, 3)).astype(F), rng.uniform(-1, 1, (B, 1)).astype(F), rng.uniform(-1, 1, (B, 3)).astype(F)


def test_numpy_twins_match_float64():
    cur, act, nxt = _rows(1)
    # three to five float32 operations on values of at most 2.25: a few ulp of that
    np.testing.assert_allclose(RU.mixed_np(cur, act, nxt), RU.mixed64(cur, act, nxt), rtol=0, atol=8 * 2.25 * 2.0 ** -24)
    params = np.array([[0.8, 0.1], [-0.4, 0.7]], F)[np.arange(6) % 2]
    c, a, n, p = (np.asarray(v, np.float64) for v in (cur, act, nxt, params))
    for t in (0, 3):
        want = -(n[:, 0] - p[:, 0]) ** 2 - p[:, 1] * a[:, 0] ** 2 - 0.05 * t * c[:, 2] ** 2
        np.testing.assert_allclose(RU.goal_step_np(cur, act, nxt, params, t), want, rtol=0, atol=8 * 4.0 * 2.0 ** -24)


def test_helper_with_a_custom_reward_on_a_tiny_case():
    """particle_util.particle_returns with the twin as the reward: N = 2, A = 2, P = 2, H = 3 on a dynamics that adds the
    action to every state component, against the same recurrence in float64; and the step counter / agent rows of
    GoalStepReward."""
    N, A, P, H = 2, 2, 2, 3
    rng = np.random.default_rng(2)
    states = rng.uniform(-1, 1, (A, 3)).astype(F)
    seq = rng.uniform(-1, 1, (N, A, H, 1)).astype(F)
    eps = rng.standard_normal((A, P, H, 3)).astype(F)
    sigma = np.full(3, 0.1, F)

    class Shift:
        handler = None
        reward = staticmethod(RU.mixed_np)

        @staticmethod
        def predict_next_state(s, a):
            return (O.f32(s) + F(0.25) * O.f32(a)).astype(F)
    got = PU.particle_returns(Shift, states, seq, eps, sigma, P)
    want = np.zeros((N, P, A))
    for n in range(N):
        for p in range(P):
            for a in range(A):
                s = states[a].astype(np.float64)
                for t in range(H):
                    nxt = s + 0.25 * float(seq[n, a, t, 0]) + sigma.astype(np.float64) * eps[a, p, t]
                    want[n, p, a] += RU.mixed64(s[None], seq[n, a, t][None], nxt[None])[0]
                    s = nxt
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    goals = np.array([[0.8, 0.1], [-0.4, 0.7]], F)
    Shift.reward = RU.GoalStepReward(goals)
    got = PU.particle_returns(Shift, states, seq, eps, sigma, P)
    assert Shift.reward.t == H
    want = np.zeros((N, P, A))
    for n in range(N):
        for p in range(P):
            for a in range(A):
                s = states[a].astype(np.float64)
                for t in range(H):
                    u = float(seq[n, a, t, 0])
                    nxt = s + 0.25 * u + sigma.astype(np.float64) * eps[a, p, t]
                    want[n, p, a] += -(nxt[0] - goals[a, 0]) ** 2 - float(goals[a, 1]) * u * u - 0.05 * t * s[2] ** 2
                    s = nxt
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)


def test_reward_program_with_the_particle_scorers_cross_compiles(L):
    for src in (RU.MIXED_REWARD, RU.PENDULUM_AS_EXECUTED, RU.NAN_ABOVE_REWARD):
        assert L.lib.bbmpc_check_user_source(L.USER_KIND_REWARD, src.encode(), 3, 1) == 0, L.lib.bbmpc_last_error()
    assert L.lib.bbmpc_check_user_source(L.USER_KIND_REWARD, RU.MIXED_REWARD.encode(), 20, 10) == 0, L.lib.bbmpc_last_error()
    assert L.lib.bbmpc_check_user_params(RU.GOAL_STEP_REWARD.encode(), 2, None, 0, 3, 1) == 0, L.lib.bbmpc_last_error()
    # the classic entry point under a parameterised declaration does not compile: the scorers call the declared form
    assert L.lib.bbmpc_check_user_params(RU.MIXED_REWARD.encode(), 2, None, 0, 3, 1) != 0
