"""What of plan gradients (include/bbmpc.h: bbmpc_plan_gradient) can be checked without a GPU: the
float64 statement of tests/plan_gradient_util.py against torch autograd (1e-10 of the largest gradient entry) and against
central differences of its own return (1e-6), on networks that cover all twelve activations, statistics on and off and
every reward mask; the activation-derivative table; refine_plan on the statement as backend; MPCPolicy's keywords; the
library's exports."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import plan_gradient_util as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = PG.cpu_cases()
MARGIN = 1e-3                      # every pre-activation of a kinked activation stays this far from the kink


def _case_inputs(case, B=2, Hq=3):
    _, dyn, rew, val, w = case
    return PG.inputs(dyn, rew, val, w, B, Hq, 2 * MARGIN)


# ---- torch twin (float64 autograd) ------------------------------------------------------------------------------------------
def _torch_act(name, x):
    import torch
    if name is None:
        return x
    if name == "tanh":
        return torch.tanh(x)
    if name == "relu":
        return torch.relu(x)
    if name == "sigmoid":
        return torch.sigmoid(x)
    if name == "elu":
        return torch.where(x > 0, x, torch.exp(torch.clamp(x, max=0.0)) - 1.0)
    if name == "selu":
        return torch.where(x > 0, PG.SELU_L * x, PG.SELU_LA * torch.exp(torch.clamp(x, max=0.0)) - PG.SELU_LA)
    if name == "softplus":
        return torch.nn.functional.softplus(x)
    if name == "softsign":
        return x / (1.0 + torch.abs(x))
    if name == "exponential":
        return torch.exp(x)
    if name == "hard_sigmoid":
        return torch.clamp(0.2 * x + 0.5, 0.0, 1.0)
    if name == "swish":
        return x * torch.sigmoid(x)
    if name == "leaky_relu":
        return torch.nn.functional.leaky_relu(x, 0.2)
    if name == "relu6":
        return torch.clamp(x, 0.0, 6.0)
    raise AssertionError(name)


def _torch_stack(net, x):
    import torch
    for w, b, a in zip(net.ws, net.bs, net.acts):
        x = _torch_act(a, x @ torch.tensor(w, dtype=torch.float64) + torch.tensor(b, dtype=torch.float64))
    return x


def _t(v):
    import torch
    return torch.tensor(np.asarray(v, np.float64), dtype=torch.float64)


def _torch_return(dyn, rew, val, w, states, seq):
    import torch
    eps = float(np.float32(1e-7))
    s = _t(states)
    total = torch.zeros(seq.shape[0], dtype=torch.float64)
    for t in range(seq.shape[1]):
        a = seq[:, t]
        x = torch.cat([s, a], 1)
        if dyn.stats is not None:
            x = (x - torch.cat([_t(dyn.stats[0]), _t(dyn.stats[2])])) / (torch.cat([_t(dyn.stats[1]), _t(dyn.stats[3])]) + eps)
        y = _torch_stack(dyn, x)
        s1 = s + (_t(dyn.stats[4]) + y * (_t(dyn.stats[5]) + eps) if dyn.stats is not None else y)
        xr = torch.cat(([s] if rew.mask & 1 else []) + ([a] if rew.mask & 2 else []) + ([s1] if rew.mask & 4 else []), 1)
        if rew.stats is not None:
            xr = (xr - _t(rew.stats[0])) / (_t(rew.stats[1]) + eps)
        r = _torch_stack(rew, xr)[:, 0]
        if rew.stats is not None:
            r = r * float(rew.stats[3][0]) + float(rew.stats[2][0])
        total = total + r
        s = s1
    if val is not None:
        xv = (s - _t(val.stats[0])) / (_t(val.stats[1]) + eps) if val.stats is not None else s
        v = _torch_stack(val, xv)[:, 0]
        if val.stats is not None:
            v = v * float(val.stats[3][0]) + float(val.stats[2][0])
        total = total + float(w) * v
    return total


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_statement_gradient_equals_autograd_and_finite_differences(case):
    import torch
    _, dyn, rew, val, w = case
    states, seq, seed, margin = _case_inputs(case)
    info = {}
    R, G = PG.value_and_grad(dyn, rew, val, w, states, seq, info=info)
    assert info["margin"] >= MARGIN, (seed, info["margin"])     # a bad seed fails here instead of hiding a mismatch
    scale = np.max(np.abs(G))
    assert scale > 1e-4 and np.all(np.isfinite(G))
    # autograd
    q = _t(seq).requires_grad_(True)
    Rt = _torch_return(dyn, rew, val, w, states, q)
    Rt.sum().backward()
    np.testing.assert_allclose(Rt.detach().numpy(), R, rtol=1e-12, atol=1e-12)
    gap = np.max(np.abs(q.grad.numpy() - G)) / scale
    print(case[0], "seed", seed, "margin %.3g" % margin, "autograd gap %.3g" % gap)
    assert gap <= 1e-10
    # central differences of the statement's own R
    h = 1e-5
    fd = np.zeros_like(G)
    base = np.asarray(seq, np.float64)
    for t in range(seq.shape[1]):
        for u in range(seq.shape[2]):
            up, dn = base.copy(), base.copy()
            up[:, t, u] += h
            dn[:, t, u] -= h
            fd[:, t, u] = (PG.value_and_grad(dyn, rew, val, w, states, up)[0] - PG.value_and_grad(dyn, rew, val, w, states, dn)[0]) / (2 * h)
    gap_fd = np.max(np.abs(fd - G)) / scale
    print(case[0], "finite-difference gap %.3g" % gap_fd)
    assert gap_fd <= 1e-6


def test_cases_cover_every_activation_mask_and_both_normalisations():
    acts = set(a for c in CASES for net in c[1:4] if net is not None for a in net.acts)
    assert acts >= set(PG.ACT_NAMES[1:])
    assert set(c[2].mask for c in CASES) == set(range(1, 8))
    assert {c[1].stats is None for c in CASES} == {True, False} and {c[2].stats is None for c in CASES} == {True, False}
    assert any(c[3] is None for c in CASES) and any(c[4] == 0.0 and c[3] is not None for c in CASES)


@pytest.mark.parametrize("name", PG.ACT_NAMES[1:])
def test_activation_derivative_table_against_autograd(name):
    import torch
    x = np.linspace(-7.3, 7.3, 293)
    for kink in PG.KINKS.get(name, ()):
        x = x[np.abs(x - kink) > 1e-3]
    y, d = PG.act_value_grad(name, x)
    xt = _t(x).requires_grad_(True)
    yt = _torch_act(name, xt)
    yt.sum().backward()
    np.testing.assert_allclose(y, yt.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(d, xt.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_kink_convention_is_the_forward_branch():
    z = np.array([0.0])
    assert PG.act_value_grad("relu", z)[1][0] == 0.0
    assert PG.act_value_grad("leaky_relu", z)[1][0] == 0.2
    assert PG.act_value_grad("relu6", z)[1][0] == 1.0 and PG.act_value_grad("relu6", np.array([6.0]))[1][0] == 1.0
    assert PG.act_value_grad("hard_sigmoid", np.array([-2.5]))[1][0] == 0.2 and PG.act_value_grad("hard_sigmoid", np.array([2.5]))[1][0] == 0.2
    src = open(os.path.join(ROOT, "blackbox_mpc_amd", "csrc", "activations_grad.hpp")).read()
    for code in ("ACT_TANH", "ACT_RELU", "ACT_SIGMOID", "ACT_ELU", "ACT_SELU", "ACT_SOFTPLUS", "ACT_SOFTSIGN", "ACT_EXPONENTIAL",
                 "ACT_HARD_SIGMOID", "ACT_SWISH", "ACT_LEAKY_RELU", "ACT_RELU6"):
        assert "case %s:" % code in src


# ---- refine_plan on the statement as backend ----------------------------------------------------------------------------------
class _StatementBackend:
    """what refine_plan asks of an Engine: plan_gradient(states [B, S], seqs [B, H, U]) -> (returns, grad)"""

    def __init__(self, case):
        _, self.dyn, self.rew, self.val, self.w = case
        self.calls = 0

    def plan_gradient(self, states, seqs):
        self.calls += 1
        R, G = PG.value_and_grad(self.dyn, self.rew, self.val, self.w, states, seqs)
        return R, G


@pytest.mark.parametrize("method", ["adam", "sgd"])
def test_refine_plan_is_monotone_and_respects_asymmetric_bounds(method):
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan
    case = CASES[0]
    be = _StatementBackend(case)
    lo, hi = np.array([-0.3, -1.0]), np.array([0.7, 0.1])
    rng = np.random.default_rng(3)
    states = rng.normal(0, 0.5, (5, 3))
    plans = rng.uniform(lo, hi, (5, 4, 2))
    r0 = be.plan_gradient(states, plans)[0]
    prev = r0
    for steps in (1, 2, 5, 9):
        out, ret = refine_plan(be, states, plans, steps, 0.05, lo, hi, method=method)
        assert out.shape == plans.shape
        assert np.all(out >= lo - 1e-12) and np.all(out <= hi + 1e-12)
        np.testing.assert_allclose(be.plan_gradient(states, out)[0], ret, rtol=1e-12, atol=1e-12)
        assert np.all(ret >= prev - 1e-12)                     # best-so-far per row: more steps are never worse
        prev = ret
    assert np.all(prev >= r0) and np.any(prev > r0 + 1e-6)


def test_refine_plan_with_zero_steps_returns_the_input():
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan
    be = _StatementBackend(CASES[1])
    rng = np.random.default_rng(4)
    states, plans = rng.normal(0, 0.5, (3, 3)), rng.uniform(-1, 1, (3, 2, 2))
    out, ret = refine_plan(be, states, plans, 0, 0.05, [-1, -1], [1, 1])
    np.testing.assert_array_equal(out, plans)
    np.testing.assert_allclose(ret, be.plan_gradient(states, plans)[0])
    with pytest.raises(ValueError):
        refine_plan(be, states, plans, 2, 0.05, [-1, -1], [1, 1], method="newton")
    with pytest.raises(ValueError):
        refine_plan(be, states, plans, -1, 0.05, [-1, -1], [1, 1])


def test_mpc_policy_keyword_validation():
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    act, obs = Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8])
    kw = dict(reward_function=pendulum_reward_function, env_action_space=act, env_observation_space=obs, true_model=True,
              dynamics_function=PendulumTrueModel(), optimizer_name="CEM", num_agents=1)
    with pytest.raises(ValueError, match="refine_steps"):
        MPCPolicy(refine_steps=-1, **kw)
    with pytest.raises(ValueError, match="refine_lr"):
        MPCPolicy(refine_steps=2, refine_lr=0.0, **kw)
    with pytest.raises(ValueError, match="learned"):           # gradients need learned dynamics and a learned reward
        MPCPolicy(refine_steps=2, **kw)


def test_library_exports_the_new_symbols(built_lib):
    lib = ctypes.CDLL(built_lib)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bbmpc.h")).read(), flags=re.S)
    from blackbox_mpc_amd import _lib as L
    for name in ("bbmpc_plan_gradient", "bbmpc_plan_gradient_dev"):
        assert re.search(r"\bint %s\(" % name, text)
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)
