"""CPU tests of plan refinement on the device: the statement of tests/plan_refine_util.py against
utils.plan_refinement.refine_plan, the clip and keep-best rules, the keyword validation and the library's exports."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import plan_gradient_util as PG
from tests import plan_refine_util as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BOUNDS = {1: (np.array([-0.4]), np.array([0.9])), 3: (np.array([-0.4, -1.0, -0.2]), np.array([0.9, 0.1, 0.6]))}


def _nets(U):
    dyn = PG.Dynamics("d-tanh20-u%d" % U, 3, U, [20], ["tanh", None], True, 41 + U)
    rew = PG.Stack("r-tanh20-u%d" % U, 3, U, 7, [20], ["tanh", None], True, 51 + U)
    val = PG.Stack("v-tanh20-u%d" % U, 3, U, 1, [20], ["tanh", None], True, 61 + U)
    return dyn, rew, val, 0.7


class _Backend:
    """what refine_plan asks of an Engine, answered by the float64 statement of the gradient"""

    def __init__(self, nets):
        self.nets = nets

    def plan_gradient(self, states, seqs):
        return PG.value_and_grad(*self.nets, states, seqs)


def _inputs(U, B=5, H=4, seed=3):
    lo, hi = BOUNDS[U]
    rng = np.random.default_rng(seed)
    return rng.normal(0, 0.5, (B, 3)).astype(F), rng.uniform(lo, hi, (B, H, U)).astype(F)


@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("steps", [0, 1, 3])
@pytest.mark.parametrize("method", ["adam", "sgd"])
def test_float64_statement_equals_refine_plan(method, steps, U):
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan
    be = _Backend(_nets(U))
    lo, hi = BOUNDS[U]
    states, plans = _inputs(U)
    want, want_ret = refine_plan(be, states, plans, steps, 0.3, lo, hi, method=method)
    got, got_ret = PR.refine(be.plan_gradient, states, plans, steps, 0.3, lo, hi, method, keep=True)
    np.testing.assert_allclose(got, want.astype(np.float64), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_ret, want_ret, rtol=0, atol=1e-12)
    if steps == 0:
        np.testing.assert_array_equal(got, plans)


@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("method", ["adam", "sgd"])
def test_the_clip_binds_on_some_elements_and_not_on_others(method, U):
    be = _Backend(_nets(U))
    lo, hi = BOUNDS[U]
    states, plans = _inputs(U, B=9)
    # Adam's first step is lr itself; plain ascent gets the lr at which the median element moves 0.15 per step
    lr = 0.3 if method == "adam" else 0.15 / float(np.median(np.abs(be.plan_gradient(states, plans)[1])))
    out, _ = PR.refine(be.plan_gradient, states, plans, 3, lr, lo, hi, method, keep=False)
    lo, hi = lo.astype(F).astype(np.float64), hi.astype(F).astype(np.float64)    # (the float32 plans carry the rounded bound)
    at_bound = (out == lo) | (out == hi)
    print(method, U, "at a bound", int(at_bound.sum()), "inside", int((~at_bound).sum()))
    assert at_bound.sum() > 0 and (~at_bound).sum() > 0
    for u in range(U):                                           # every dimension against its own bound
        assert np.all(out[..., u] >= lo[u]) and np.all(out[..., u] <= hi[u])


def test_a_nan_return_never_replaces_the_best():
    x0, x1 = np.zeros((3, 2, 1)), np.ones((3, 2, 1))
    best, best_ret = PR.keep_best(x0, np.array([1.0, np.nan, -2.0]), None, None)
    np.testing.assert_array_equal(best, x0)
    best, best_ret = PR.keep_best(x1, np.array([np.nan, 5.0, -1.0]), best, best_ret)
    np.testing.assert_array_equal(best[:, 0, 0], [0.0, 0.0, 1.0])     # row 0: NaN does not replace; row 1: nothing beats a stored NaN
    np.testing.assert_array_equal(best_ret, [1.0, np.nan, -1.0])

    calls = []

    def nan_after_the_first(states, plans):
        calls.append(1)
        ret = np.full(plans.shape[0], 1.0 if len(calls) == 1 else np.nan)
        return ret, np.ones(plans.shape)
    out, ret = PR.refine(nan_after_the_first, None, x0.astype(F), 3, 0.1, [-1.0], [1.0], "sgd", keep=True)
    assert len(calls) == 4
    np.testing.assert_array_equal(out, x0)
    np.testing.assert_array_equal(ret, np.ones(3))


def test_a_non_finite_step_counts_as_zero():
    x = np.array([[[0.25], [0.5]]])
    g = np.array([[[np.inf], [np.nan]]])
    for dt in (np.float64, np.float32):
        for method in ("adam", "sgd"):
            out, _, _ = PR.update(x, g, np.zeros_like(x), np.zeros_like(x), 1, 0.1, [-1.0], [1.0], method, dt)
            np.testing.assert_array_equal(out, x.astype(dt))


def test_float32_restatement_stays_close_to_float64():
    be = _Backend(_nets(3))
    lo, hi = BOUNDS[3]
    states, plans = _inputs(3)
    g = be.plan_gradient(states, plans)[1]
    z = np.zeros_like(g)
    for method in ("adam", "sgd"):
        a = PR.update(plans, g, z, z, 1, 0.05, lo, hi, method, np.float64)[0]
        b = PR.update(plans, g, z, z, 1, 0.05, lo, hi, method, np.float32)[0]
        assert b.dtype == F and 0 < np.max(np.abs(a - b)) < 1e-6
    c1, c2 = PR.bias_correction(3, np.float32)
    assert abs(float(c1) - (1 - 0.9 ** 3)) < 1e-6 and abs(float(c2) - (1 - 0.999 ** 3)) < 1e-6


def _pendulum_kw():
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    act, obs = Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8])
    return act, obs, PendulumTrueModel(), pendulum_reward_function


def test_cem_optimizer_keyword_validation():
    from blackbox_mpc_amd.optimizers import CEMOptimizer
    act, obs, _, _ = _pendulum_kw()
    kw = dict(env_action_space=act, env_observation_space=obs, planning_horizon=5, population_size=48, num_elite=8, num_agents=1)
    for bad in (dict(grad_steps=-1), dict(grad_steps=65), dict(grad_steps=1.5), dict(grad_steps=True)):
        with pytest.raises(ValueError, match="grad_steps"):
            CEMOptimizer(**kw, **bad)
    for bad in (dict(grad_candidates=-1), dict(grad_candidates=49), dict(grad_candidates=2.0)):
        with pytest.raises(ValueError, match="grad_candidates"):
            CEMOptimizer(grad_steps=1, **kw, **bad)
    for bad in (dict(grad_lr=0.0), dict(grad_lr=-1.0), dict(grad_lr=float("inf")), dict(grad_lr=float("nan")), dict(grad_lr="x")):
        with pytest.raises(ValueError, match="grad_lr"):
            CEMOptimizer(grad_steps=1, **kw, **bad)
    with pytest.raises(ValueError, match="grad_method"):
        CEMOptimizer(grad_steps=1, grad_method="newton", **kw)
    assert CEMOptimizer(**kw)._grad_refine is None
    assert CEMOptimizer(grad_steps=2, grad_lr=0.1, grad_method="sgd", grad_candidates=21, **kw)._grad_refine == (2, 0.1, "sgd", 21)


def test_mpc_policy_keyword_validation():
    from blackbox_mpc_amd.policies import MPCPolicy
    act, obs, model, reward = _pendulum_kw()
    kw = dict(reward_function=reward, env_action_space=act, env_observation_space=obs, true_model=True, dynamics_function=model,
              optimizer_name="CEM", num_agents=1, planning_horizon=5, population_size=48, num_elite=8)
    with pytest.raises(ValueError, match="grad_steps"):
        MPCPolicy(grad_steps=-1, **kw)
    with pytest.raises(ValueError, match="learned"):            # gradients need learned dynamics and a learned reward
        MPCPolicy(grad_steps=2, **kw)
    with pytest.raises(ValueError, match="refine_device"):
        MPCPolicy(refine_device=1, **kw)
    with pytest.raises(TypeError):                               # only CEM has candidates to refine
        MPCPolicy(grad_steps=2, **dict(kw, optimizer_name="PI2"))


def test_refine_plan_device_validation():
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan_device
    s, q = np.zeros((2, 3), F), np.zeros((2, 4, 1), F)
    with pytest.raises(ValueError, match="method"):
        refine_plan_device(object(), s, q, 2, 0.05, method="newton")
    with pytest.raises(ValueError, match="steps"):
        refine_plan_device(object(), s, q, -1, 0.05)
    with pytest.raises(ValueError, match="lr"):
        refine_plan_device(object(), s, q, 2, 0.0)
    with pytest.raises(TypeError):
        refine_plan_device(object(), s, q, 2, 0.05)


def test_library_exports_the_new_symbols(built_lib):
    lib = ctypes.CDLL(built_lib)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bbmpc.h")).read(), flags=re.S)
    from blackbox_mpc_amd import _lib as L
    for name in ("bbmpc_refine_plans", "bbmpc_refine_plans_dev", "bbmpc_set_grad_refine", "bbmpc_get_grad_refine"):
        assert re.search(r"\bint %s\(" % name, text)
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)
