"""CPU checks of the float64 restatement of the control step's tail (tests/tail_util.py) and of the designed inputs the
GPU tests (tests/test_gpu_control_step_tail.py) feed it: the helper agrees with the oracle's OptimizerBase.call, the
designed bounds / noise sets exercise the clip on both sides and tell quirk Q7 from its fix by the reference alone, and the
documented production draw is what the helper says it is."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import philox_np as P
from tests import tail_util as T

F = np.float32


class _Fixed(O.OptimizerBase):
    """OptimizerBase with a given solution: only the tail (optimizer_base.py:82-94) runs"""

    def __init__(self, evaluator, lo, hi, action):
        super().__init__(evaluator, lo, hi, 1, action.shape[0], None)
        self._action = action

    def _optimize(self, state, noise):
        return self._action.copy()


class _DummyEvaluator:
    def predict_next_state(self, s, a):
        return s

    def evaluate_next_reward(self, s, n, a):
        return np.zeros((s.shape[0],), F)


def _action_families(lo, hi, A, seed):
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    rng = np.random.default_rng(seed)
    U = lo.shape[0]
    return {"lo": np.tile(lo, (A, 1)), "hi": np.tile(hi, (A, 1)), "mid": np.tile((lo + hi) / F(2), (A, 1)).astype(F),
            "random": (lo + rng.random((A, U)).astype(F) * (hi - lo)).astype(F)}


# (name, lo, hi, A): every bounds / noise set of the GPU tests at the size the conditions are stated for
SETS = [("pendulum-" + k, v[0], v[1], 9) for k, v in T.PENDULUM_BOUNDS.items()] + \
       [("mlp-U2", T.MLP_BOUNDS[2][0], T.MLP_BOUNDS[2][1], 3), ("mlp-U6", T.MLP_BOUNDS[6][0], T.MLP_BOUNDS[6][1], 3),
        ("mlp-U64",) + T.wide_bounds(64) + (2,), ("mlp-U125",) + T.wide_bounds(125) + (2,),       # (A U = 250: 5 divides it)
        ("user-U2", T.MLP_BOUNDS[2][0], T.MLP_BOUNDS[2][1], 9)]
XI_SEEDS = (0, 2)                     # the control steps that run with noise on


@pytest.mark.parametrize("name,lo,hi,A", SETS, ids=[s[0] for s in SETS])
def test_helper_agrees_with_the_oracle_tail(name, lo, hi, A):
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    U = lo.shape[0]
    pend = name.startswith("pendulum")
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True)) if pend else _DummyEvaluator()
    states = O.pendulum_start_states(A) if pend else np.zeros((A, 3), F)
    for fam, action in _action_families(lo, hi, A, 7).items():
        for seed in XI_SEEDS:
            xi = T.designed_xi(A, U, seed)
            got, nxt, rew = _Fixed(ev, lo, hi, action).call(states, None, exploration_noise=xi)
            T.check_action(got, action, xi, lo, hi, False, what="%s %s" % (name, fam))
            if pend:          # the record the oracle returns is the model step of ITS noisy action
                np.testing.assert_array_equal(nxt, ev.predict_next_state(states, got))
            quiet, _, _ = _Fixed(ev, lo, hi, action).call(states, None)
            np.testing.assert_array_equal(quiet, action)
    # in-distribution sanity of the helper itself: zero noise and zero midpoint leave an in-range action alone
    np.testing.assert_array_equal(T.exploration(action, np.zeros((A, U)), lo, hi, True), action.astype(np.float64))


@pytest.mark.parametrize("name,lo,hi,A", SETS, ids=[s[0] for s in SETS])
def test_designed_inputs_exercise_the_clip_and_tell_q7_from_its_fix(name, lo, hi, A):
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    U = lo.shape[0]
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    mid = (hi64 + lo64) / 2
    for fam, action in _action_families(lo, hi, A, 7).items():
        for seed in XI_SEEDS:
            xi = T.designed_xi(A, U, seed)
            assert np.sum(np.abs(xi) == F(T.FORCE)) == 2 and np.sum(np.abs(np.abs(xi) - 2) < 1e-3) >= 2 and np.sum(np.abs(xi) < 1e-2) >= 1
            indist = np.abs(xi) < 2
            for fix in (False, True):
                raw = T.exploration_unclipped(action, xi, lo, hi, fix)
                tol = T.action_atol(action, xi, lo, hi, fix)
                at_hi, at_lo = raw > hi64 + tol, raw < lo64 - tol
                inside = (raw > lo64 + tol) & (raw < hi64 - tol)
                what = "%s %s fix_q7=%s step %d" % (name, fam, fix, seed)
                # whatever the optimizer returns (all four families): something clips at hi and something at lo
                assert at_hi.any() and at_lo.any(), what
                if name in ("pendulum-asym", "pendulum-pos") and not fix:
                    # Q7 sets where draws inside (-2, 2) cannot reach lo: the midpoint exceeds 2 sd, the noise is positive
                    assert not (at_lo & indist).any(), what
                if name == "pendulum-pos" and not fix:
                    # lo > 0: Q7's midpoint alone (= hi - lo) saturates every in-distribution row whose action is not within
                    # 2 sd of lo -- reference behaviour, pinned here and checked on the device next to its FIX_Q7 twin
                    far = indist & (action.astype(np.float64) > lo64 + 2 * T.exploration_std(lo, hi))
                    assert np.all(T.exploration(action, xi, lo, hi, False)[far] == hi64[0]), what
                elif fam in ("mid", "random"):
                    assert inside.any(), what          # an action strictly inside the bounds: some element stays inside
            if np.all(mid == 0):
                continue                               # pendulum-sym: Q7 and its fix coincide, nothing to tell apart
            q7, fx = T.exploration(action, xi, lo, hi, False), T.exploration(action, xi, lo, hi, True)
            tol = np.maximum(T.action_atol(action, xi, lo, hi, False), T.action_atol(action, xi, lo, hi, True))
            unclipped = (fx > lo64) & (fx < hi64) & (np.broadcast_to(mid, fx.shape) != 0)
            if fam in ("mid", "random"):
                assert unclipped.sum() >= (A * U) // 3, what
                assert np.sum((np.abs(q7 - fx) > 100 * tol) & unclipped) * 2 >= unclipped.sum(), what


@pytest.mark.parametrize("U", [1, 4, 5, 6, 9])
def test_production_exploration_draw(U):
    seed, A, steps = 0x1234567890ABCDEF, 4, 4
    xs = np.stack([T.exploration_xi(seed, t, A, U) for t in range(steps)])
    assert xs.shape == (steps, A, U) and xs.dtype == F
    assert np.all(np.abs(xs) < 2)                                          # strictly inside (-2, 2)
    assert np.unique(xs).size == xs.size                                   # distinct per agent, per u and per step
    # ... and keyed by the GLOBAL agent: a shard's rows are the unsharded rows
    np.testing.assert_array_equal(T.exploration_xi(seed, 2, 2, U, agent_offset=2), xs[2, 2:])
    # the documented counter, spelled out: (0, ga * ceil(U/4) + (u >> 2), control step, 10 << 16), output word u & 3
    q = (U + 3) // 4
    for t, a, u in ((0, 0, 0), (3, 3, U - 1), (1, 2, U // 2)):
        w = P.philox4x32_10(0, a * q + (u >> 2), t, 10 << 16, seed & 0xFFFFFFFF, seed >> 32)[u & 3]
        assert xs[t, a, u] == P.trunc_normal(np.asarray(w, np.uint32).reshape(1))[0]


def test_shift_left():
    m = np.arange(2 * 4 * 3, dtype=F).reshape(2, 4, 3)
    s = T.shift_left(m)
    np.testing.assert_array_equal(s[:, :3], m[:, 1:])
    np.testing.assert_array_equal(s[:, 3], m[:, 3])
    # the oracle's PI2 leaves exactly this behind (pi2.py:92-93)
    N, A, H = 8, 2, 4
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
    o = O.PI2(ev, [-2.0], [2.0], horizon=H, max_iterations=2, population=N, num_agents=A)
    rng = np.random.default_rng(1)
    o.call(O.pendulum_start_states(A), {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(2)]})
    np.testing.assert_array_equal(o.prev, T.shift_left(o.trace[-1]["mean"]))
