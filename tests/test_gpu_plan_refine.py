"""GPU tests of plan refinement on the device (bbmpc_refine_plans, bbmpc_set_grad_refine) through the C
ABI and the Python layers.

Tolerances come from the statement (tests/plan_refine_util.py), never from the kernel: one step is held to 4 x the gap between
the float32 restatement and float64 of the same update on the same device gradient plus one ulp of the action; three steps to
4 x the gap of the float32 chain (float32 statement gradient, float32 update) to the float64 chain.  Tanh networks: no kinks.
Measured on an MI355X (B = 37, Hq = 5): one step, device gap = the float32 restatement's own gap in all four cases (Adam 2.0e-6
and 2.1e-6 at U = 1 and 3, bound 8.2e-6 and 8.4e-6; SGD 3.7e-8 and 4.4e-8, bound 2.1e-7 and 3.0e-7); three steps, Adam 2.3e-6
(bound 9.3e-6 and 9.5e-6), SGD 6.0e-8 and 1.2e-7 (bound 2.4e-7 and 3.0e-7)."""
import ctypes

import numpy as np
import pytest

from tests import plan_gradient_util as PG
from tests import plan_refine_util as PR
from tests import reward_mlp_util as R

pytestmark = pytest.mark.gpu
F = np.float32
B, HQ = 37, 5
# asymmetric per-dimension bounds, exactly representable in float32 (the handle keeps float32 bounds)
BOUNDS = {1: (np.array([-0.5], F), np.array([0.875], F)), 3: (np.array([-0.5, -1.0, -0.25], F), np.array([0.875, 0.125, 0.625], F))}


def _nets(U):
    dyn = PG.Dynamics("d-tanh20-u%d" % U, 3, U, [20], ["tanh", None], True, 41 + U)
    rew = PG.Stack("r-tanh20-u%d" % U, 3, U, 7, [20], ["tanh", None], True, 51 + U)
    val = PG.Stack("v-tanh20-u%d" % U, 3, U, 1, [20], ["tanh", None], True, 61 + U)
    return dyn, rew, val, 0.7


NETS = {1: _nets(1), 3: _nets(3)}


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _engine(L, U, opt=None, A=1, H=1, dynamics=None, rew=None, nets=True, **kw):
    from blackbox_mpc_amd.engine import Engine
    dyn, rnet, vnet, w = NETS[U]
    lo, hi = BOUNDS[U]
    eng = Engine(L.OPT_NONE if opt is None else opt, L.DYN_MLP if dynamics is None else dynamics, L.REW_MLP if rew is None else rew,
                 lo, hi, dim_s=3, num_agents=A, planning_horizon=H, **kw)
    if nets and dynamics is None:
        eng.set_mlp(dyn.ws, dyn.bs, dyn.codes(), dyn.stats)
        if rew is None:
            eng.set_reward_mlp(rnet.ws, rnet.bs, rnet.codes(), rnet.mask, rnet.stats)
            eng.set_terminal_value_mlp(vnet.ws, vnet.bs, vnet.codes(), vnet.stats, w)
    return eng


@pytest.fixture(scope="module")
def data():
    """per U: states, plans inside the bounds (margin of the kinked activations asserted by PG.inputs: none here, tanh)"""
    out = {}
    for U in (1, 3):
        lo, hi = BOUNDS[U]
        states, seq, _, margin = PG.inputs(*NETS[U], B, HQ, 1e-4, base_seed=10 + U)
        assert margin >= 1e-4
        plans = (lo + (seq + 1) * F(0.5) * (hi - lo)).astype(F)          # uniform(-1, 1) mapped into [lo, hi]
        assert np.all(plans >= lo) and np.all(plans <= hi)
        out[U] = (states, plans)
    return out


def _statement(U, dt):
    return lambda s, q: PG.value_and_grad(*NETS[U], s, q, dt=dt)


def _lr(method, g):
    """Adam's first step is lr itself; plain ascent gets the lr at which the median element moves 0.15: the clip binds on some
    elements and not on others (test_plan_refine_cpu.py chooses the same way)"""
    return 0.3 if method == "adam" else 0.15 / float(np.median(np.abs(g)))


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("method", ["adam", "sgd"])
def test_one_step_teacher_forced(L, data, method, U):
    eng = _engine(L, U)
    states, plans = data[U]
    lo, hi = BOUNDS[U]
    _, g = eng.plan_gradient(states, plans)
    lr = F(_lr(method, g))                                       # the float32 value the C side receives
    z = np.zeros_like(g)
    want = PR.update(plans, g, z, z, 1, float(lr), lo, hi, method, np.float64)[0]
    x32 = PR.update(plans, g, z, z, 1, lr, lo, hi, method, np.float32)[0]
    gap32 = float(np.max(np.abs(x32 - want)))
    tol = 4 * gap32 + float(np.spacing(F(np.max(np.abs(np.concatenate([lo, hi]))))))
    out, _ = eng.refine_plans(states, plans, 1, lr, method=method, keep_best=False)
    gap = float(np.max(np.abs(out - want)))
    at_bound = (out == lo) | (out == hi)
    print(method, "U", U, "device gap %.3g, float32 restatement gap %.3g, tolerance %.3g; at a bound %d, inside %d"
          % (gap, gap32, tol, at_bound.sum(), (~at_bound).sum()))
    assert out.dtype == F and out.shape == plans.shape
    assert at_bound.sum() > 0 and (~at_bound).sum() > 0
    assert gap <= tol


@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("method", ["adam", "sgd"])
def test_three_steps_against_the_float64_chain(L, data, method, U):
    eng = _engine(L, U)
    states, plans = data[U]
    lo, hi = BOUNDS[U]
    lr = F(_lr(method, _statement(U, np.float64)(states, plans)[1])) * F(0.25)     # (smaller steps: most elements stay inside)
    want, _ = PR.refine(_statement(U, np.float64), states, plans, 3, float(lr), lo, hi, method, keep=False, dt=np.float64)
    x32, _ = PR.refine(_statement(U, np.float32), states, plans, 3, lr, lo, hi, method, keep=False, dt=np.float32)
    gap32 = float(np.max(np.abs(x32 - want)))
    assert gap32 > 0
    out, ret = eng.refine_plans(states, plans, 3, lr, method=method, keep_best=False)
    gap = float(np.max(np.abs(out - want)))
    print(method, "U", U, "three steps: device gap %.3g, float32 chain gap %.3g, tolerance %.3g" % (gap, gap32, 4 * gap32))
    assert gap <= 4 * gap32
    np.testing.assert_array_equal(ret, eng.plan_gradient(states, out)[0])       # returns_out scores the last iterate


# ---- 2. keep-best ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["adam", "sgd"])
def test_keep_best(L, data, method):
    U = 3
    eng = _engine(L, U)
    states, plans = data[U]
    lo, hi = BOUNDS[U]
    r0, g = eng.plan_gradient(states, plans)
    lr = _lr(method, g)
    out, ret = eng.refine_plans(states, plans, 4, lr, method=method, keep_best=True)
    assert np.all(ret >= r0)
    assert np.any(ret > r0)
    np.testing.assert_array_equal(ret, eng.plan_gradient(states, out)[0])
    assert np.all(out >= lo) and np.all(out <= hi)
    out0, ret0 = eng.refine_plans(states, plans, 0, lr, method=method, keep_best=True)
    np.testing.assert_array_equal(out0, plans)
    np.testing.assert_array_equal(ret0, r0)
    # the rows keep-best took are iterates of the loop without it: more steps are never worse
    _, ret2 = eng.refine_plans(states, plans, 2, lr, method=method, keep_best=True)
    assert np.all(ret >= ret2) and np.all(ret2 >= r0)


def test_refine_plan_device_follows_refine_plan(L, data):
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan, refine_plan_device
    U = 1
    eng = _engine(L, U)
    states, plans = data[U]
    lo, hi = BOUNDS[U]
    want, want_ret = refine_plan(eng, states, plans, 3, 0.05, lo, hi)
    x64, _ = PR.refine(_statement(U, np.float64), states, plans, 3, 0.05, lo, hi, "adam", keep=False)
    x32, _ = PR.refine(_statement(U, np.float32), states, plans, 3, F(0.05), lo, hi, "adam", keep=False, dt=np.float32)
    tol = 4 * float(np.max(np.abs(x32 - x64)))
    got, got_ret = refine_plan_device(eng, states, plans, 3, 0.05)
    gap = float(np.max(np.abs(got.astype(np.float64) - want)))
    print("refine_plan_device against refine_plan: plan gap %.3g, tolerance %.3g" % (gap, tol))
    assert got.dtype == plans.dtype and got_ret.dtype == np.float64
    assert np.all(got_ret >= eng.plan_gradient(states, plans)[0])
    assert gap <= tol


def test_non_finite_rules_on_the_device(L, data):
    """k_refine_step: a non-finite step element counts as 0; k_refine_keep_best: `returns > best_ret` is false for NaN.  Rows
    whose start state holds a NaN or an Inf have a non-finite return and gradient at every iterate."""
    U = 3
    eng = _engine(L, U)
    states, plans = data[U]
    bad = states.copy()
    bad[3, 1], bad[20, 0] = np.nan, np.inf
    rows = [3, 20]
    ok = np.setdiff1d(np.arange(B), rows)
    r, g = eng.plan_gradient(bad, plans)
    assert not np.any(np.isfinite(r[rows])) and not np.any(np.isfinite(g[rows]))
    for method in ("adam", "sgd"):
        want, want_r = eng.refine_plans(states, plans, 3, 0.1, method=method, keep_best=False)
        out, ret = eng.refine_plans(bad, plans, 3, 0.1, method=method, keep_best=False)
        np.testing.assert_array_equal(out[rows], plans[rows])   # every step of these rows was 0
        np.testing.assert_array_equal(out[ok], want[ok])
        assert not np.any(np.isfinite(ret[rows]))
        want, want_r = eng.refine_plans(states, plans, 3, 0.1, method=method, keep_best=True)
        out, ret = eng.refine_plans(bad, plans, 3, 0.1, method=method, keep_best=True)
        np.testing.assert_array_equal(out[rows], plans[rows])   # the first call's plan stays: nothing is greater than NaN
        assert not np.any(np.isfinite(ret[rows]))
        np.testing.assert_array_equal(out[ok], want[ok])
        np.testing.assert_array_equal(ret[ok], want_r[ok])
    # lr * step overflowing to Inf is no non-finite STEP: the element goes to its bound
    big = float(np.finfo(F).max)
    out, ret = eng.refine_plans(states, plans, 2, big, method="sgd", keep_best=True)
    lo, hi = BOUNDS[U]
    assert np.all(np.isfinite(out)) and np.all(out >= lo) and np.all(out <= hi) and np.all(ret >= eng.plan_gradient(states, plans)[0])


def test_refine_plan_device_through_the_evaluator(L, data):
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan_device
    act, obs, handler, rew = _models()
    ev = DeterministicTrajectoryEvaluator(rew, handler)
    rng = np.random.default_rng(2)
    states, plans = rng.normal(0, 0.5, (B, 3)).astype(F), rng.uniform(act.low, act.high, (B, HQ, 1)).astype(F)
    r0 = ev.value_and_gradient(states[:1], plans[:1, None])[0]
    out, ret = ev.refine_plans_rows(states, plans, 3, 0.05)
    out2, ret2 = refine_plan_device(ev, states, plans, 3, 0.05)
    np.testing.assert_array_equal(out, out2)
    np.testing.assert_array_equal(ret.astype(np.float64), ret2)
    assert out2.dtype == plans.dtype and ret2.dtype == np.float64 and ret2[0] >= r0[0, 0]
    assert np.all(out >= act.low) and np.all(out <= act.high)   # the evaluator's engine carries the action space's bounds
    from blackbox_mpc_amd.engine import Engine
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_MLP, act.low, act.high, dim_s=3, num_agents=1, planning_horizon=1)
    dn = handler._dynamics_function
    eng.set_mlp(dn.weights, dn.biases, dn.activation_codes, handler.normalization_stats())
    eng.set_reward_mlp(rew.weights, rew.biases, rew.activation_codes, rew.input_mask, rew.normalization_stats())
    want, want_r = eng.refine_plans(states, plans, 3, 0.05)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(ret, want_r)
    with pytest.raises(ValueError):
        ev.refine_plans_rows(states, plans[:, :, 0], 3, 0.05)


# ---- 3. determinism, bounds of writing --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [False, True])
def test_equal_bits_across_runs_and_across_a_batch_split(L, data, keep):
    U = 3
    eng = _engine(L, U)
    states, plans = data[U]
    a, ra = eng.refine_plans(states, plans, 3, 0.1, keep_best=keep)
    b, rb = eng.refine_plans(states, plans, 3, 0.1, keep_best=keep)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ra, rb)
    p, rp = eng.refine_plans(states[:16], plans[:16], 3, 0.1, keep_best=keep)
    q, rq = eng.refine_plans(states[16:], plans[16:], 3, 0.1, keep_best=keep)
    np.testing.assert_array_equal(np.concatenate([p, q]), a)
    np.testing.assert_array_equal(np.concatenate([rp, rq]), ra)


@pytest.mark.parametrize("U", [1, 3])                          # row length 5 (scalar traffic) and 15 x 37 (no float4 either); 16 rows: float4
def test_rows_behind_the_batch_and_guard_bands_are_not_written(L, data, U):
    import torch
    eng = _engine(L, U)
    states, plans = data[U]
    for rows in (B, 16):
        want, want_r = eng.refine_plans(states[:rows], plans[:rows], 2, 0.1, keep_best=True)
        d_s = torch.tensor(states[:rows], device="cuda")
        d_q = torch.full((rows + 8, HQ, U), float("nan"), device="cuda")
        d_q[:rows] = torch.tensor(plans[:rows], device="cuda")
        d_r = torch.full((rows + 8,), float("nan"), device="cuda")
        torch.cuda.synchronize()
        eng.refine_plans_dev(d_s.data_ptr(), d_q.data_ptr(), rows, HQ, 2, 0.1, "adam", True, d_r.data_ptr())
        eng.synchronize()
        np.testing.assert_array_equal(d_q[:rows].cpu().numpy(), want)
        np.testing.assert_array_equal(d_r[:rows].cpu().numpy(), want_r)
        assert bool(torch.isnan(d_q[rows:]).all()) and bool(torch.isnan(d_r[rows:]).all())
        d_q[:rows] = torch.tensor(plans[:rows], device="cuda")   # returns_out may be NULL
        torch.cuda.synchronize()
        eng.refine_plans_dev(d_s.data_ptr(), d_q.data_ptr(), rows, HQ, 2, 0.1, "adam", False, 0)
        eng.synchronize()
        np.testing.assert_array_equal(d_q[:rows].cpu().numpy(), eng.refine_plans(states[:rows], plans[:rows], 2, 0.1, keep_best=False)[0])
        assert bool(torch.isnan(d_q[rows:]).all())


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def _raises(L, code, fn):
    with pytest.raises(L.BBMPCError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


CEM = dict(A=2, H=HQ, population_size=48, num_elite=8, max_iterations=2, seed=11)


def test_refine_plans_refusals_leave_the_handle_computing(L, data):
    from blackbox_mpc_amd.engine import Engine
    U = 1
    states, plans = data[U]
    s, q = states[:16], plans[:16]
    e = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=1)
    assert "BBMPC_DYN_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: e.refine_plans(s, q, 2, 0.1))
    e = _engine(L, U, rew=L.REW_PENDULUM)
    assert "BBMPC_REW_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: e.refine_plans(s, q, 2, 0.1))
    e = _engine(L, U, nets=False)
    assert "bbmpc_set_mlp" in _raises(L, L.E_STATE, lambda: e.refine_plans(s, q, 2, 0.1))
    e = _engine(L, U)
    good = e.refine_plans(s, q, 2, 0.1)[0]
    dyn = NETS[U][0]
    e.set_mlp_ensemble([(dyn.ws, dyn.bs), (dyn.ws, dyn.bs)])
    assert "ensemble" in _raises(L, L.E_UNSUPPORTED, lambda: e.refine_plans(s, q, 2, 0.1))
    e.set_mlp_ensemble([])
    out = q.copy()
    ok = (L.ptr(s), L.ptr(out), 16, HQ, 2, 0.1, 0, 1, None)
    for i, bad in ((0, None), (1, None), (2, 0), (3, 0), (3, 4097), (4, -1), (4, 65), (5, 0.0), (5, -0.1), (5, float("nan")),
                   (5, float("inf")), (6, 2), (6, -1), (7, 2), (7, -1)):
        args = list(ok)
        args[i] = bad
        assert L.lib.bbmpc_refine_plans(e._h, *args) == L.E_INVALID, (i, bad)
        assert L.lib.bbmpc_refine_plans_dev(e._h, *args) == L.E_INVALID, (i, bad)
    np.testing.assert_array_equal(out, q)
    assert L.lib.bbmpc_refine_plans_dev(e._h, ctypes.c_void_p(8), ctypes.c_void_p(8), 1 << 24, 4096, 1, 0.1, 0, 0, None) == L.E_UNSUPPORTED
    assert "2^31" in L.lib.bbmpc_last_error().decode()
    np.testing.assert_array_equal(e.refine_plans(s, q, 2, 0.1)[0], good)
    with pytest.raises(ValueError):
        e.refine_plans(s, q, 2, 0.1, method="newton")
    with pytest.raises(ValueError):
        e.refine_plans(s, q[:, :, None], 2, 0.1)


def test_set_grad_refine_refusals_leave_the_handle_as_it_was(L, data, monkeypatch):
    from blackbox_mpc_amd.engine import Engine
    U = 1
    states = data[U][0][:2]
    dyn = NETS[U][0]
    # an optimizer other than CEM
    e = _engine(L, U, opt=L.OPT_PI2, A=2, H=HQ, population_size=48, max_iterations=2)
    assert "CEM" in _raises(L, L.E_UNSUPPORTED, lambda: e.set_grad_refine(2, 0.1))
    assert np.all(np.isfinite(e.optimize(states)[0]))
    # handles bbmpc_plan_gradient would refuse
    e = Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=2, planning_horizon=HQ, population_size=48,
               num_elite=8, max_iterations=2)
    assert "BBMPC_DYN_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: e.set_grad_refine(2, 0.1))
    assert e.get_grad_refine()[0] == 0 and np.all(np.isfinite(e.optimize(states)[0]))
    e = _engine(L, U, opt=L.OPT_CEM, rew=L.REW_PENDULUM, **CEM)
    assert "BBMPC_REW_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: e.set_grad_refine(2, 0.1))
    # ... particles on that handle: refused by name, in this order of the two calls
    e.set_particles(4, [0.01, 0.01, 0.01])
    assert "particles" in _raises(L, L.E_UNSUPPORTED, lambda: e.set_grad_refine(2, 0.1))
    assert np.all(np.isfinite(e.optimize(states)[0]))
    # ... and in the other order, on a handle with the setting on
    e = _engine(L, U, opt=L.OPT_CEM, **CEM)
    e.set_grad_refine(2, 0.1, "sgd", 21)
    assert e.get_grad_refine() == (2, F(0.1), "sgd", 21)
    assert "bbmpc_set_grad_refine" in _raises(L, L.E_UNSUPPORTED, lambda: e.set_particles(4, [0.01, 0.01, 0.01]))
    assert "ensemble" in _raises(L, L.E_UNSUPPORTED, lambda: e.set_mlp_ensemble([(dyn.ws, dyn.bs), (dyn.ws, dyn.bs)]))
    assert e.get_grad_refine() == (2, F(0.1), "sgd", 21)
    # an ensemble first
    e2 = _engine(L, U, opt=L.OPT_CEM, **CEM)
    e2.set_mlp_ensemble([(dyn.ws, dyn.bs), (dyn.ws, dyn.bs)])
    assert "ensemble" in _raises(L, L.E_UNSUPPORTED, lambda: e2.set_grad_refine(2, 0.1))
    # log-variance heads, in both orders
    hw, hb = np.zeros((20, 3), F), np.zeros(3, F)
    head = lambda h: h.set_mlp_logvar_head([(hw, hb)], np.full(3, -5.0, F), np.full(3, 1.0, F))     # noqa: E731
    assert "bbmpc_set_grad_refine" in _raises(L, L.E_UNSUPPORTED, lambda: head(e))
    assert e.get_grad_refine() == (2, F(0.1), "sgd", 21)
    e5 = _engine(L, U, opt=L.OPT_CEM, **CEM)
    head(e5)
    assert "log-variance" in _raises(L, L.E_UNSUPPORTED, lambda: e5.set_grad_refine(2, 0.1))
    assert e5.get_grad_refine()[0] == 0 and np.all(np.isfinite(e5.optimize(states)[0]))
    # invalid arguments keep the setting
    for args in ((-1, 0.1, 0, 0), (65, 0.1, 0, 0), (2, 0.0, 0, 0), (2, float("nan"), 0, 0), (2, 0.1, 2, 0), (2, 0.1, 0, -1), (2, 0.1, 0, 49)):
        assert L.lib.bbmpc_set_grad_refine(e._h, *args) == L.E_INVALID, args
    assert e.get_grad_refine() == (2, F(0.1), "sgd", 21)
    before = e.optimize(states)
    assert np.all(np.isfinite(before[0]))
    # networks not yet installed: at the control step
    e3 = _engine(L, U, opt=L.OPT_CEM, nets=False, **CEM)
    e3.set_grad_refine(1, 0.1)
    assert "bbmpc_set_mlp" in _raises(L, L.E_STATE, lambda: e3.optimize(states))
    # a sharded population
    monkeypatch.setenv("BBMPC_POPSHARD_LOOPBACK", "2")
    e4 = _engine(L, U, opt=L.OPT_CEM, **CEM)
    assert "sharded" in _raises(L, L.E_UNSUPPORTED, lambda: e4.set_grad_refine(2, 0.1))
    assert np.all(np.isfinite(e4.optimize(states)[0]))


# ---- 5. in the loop -------------------------------------------------------------------------------------------------------------
def _columns_refined(L, eng, states, cols, steps, lr, method):
    """refine_plans_dev(keep_best=False) on candidate columns cols [M, A, H, U] of agents' states [A, S] -> [M, A, H, U]"""
    import torch
    M, A, H, U = cols.shape
    rows = np.ascontiguousarray(np.transpose(cols, (1, 0, 2, 3))).reshape(A * M, H, U)       # row a * M + c
    d_q = torch.tensor(rows, device="cuda")
    d_s = torch.tensor(np.repeat(states, M, axis=0), device="cuda")
    torch.cuda.synchronize()
    eng.refine_plans_dev(d_s.data_ptr(), d_q.data_ptr(), A * M, H, steps, lr, method, False, 0)
    eng.synchronize()
    return np.transpose(d_q.cpu().numpy().reshape(A, M, H, U), (1, 0, 2, 3))


def _model_returns(eng, U, states, cols):
    """forward-only model returns of candidates cols [M, A, H, U] -> [M, A]"""
    M, A, H, _ = cols.shape
    rows = cols.reshape(M * A, H, U)
    st, rews = eng.predict_trajectories(np.tile(states, (M, 1)), rows)
    want = R.returns(rews.astype(np.float64)) + NETS[U][3] * eng.evaluate_terminal_value(st[:, -1]).astype(np.float64)
    return want.reshape(M, A)


@pytest.mark.parametrize("M", [21, 0])
@pytest.mark.parametrize("U,method", [(1, "adam"), (3, "sgd")])
def test_in_the_loop_refines_the_last_columns_only(L, data, U, method, M):
    states = data[U][0][:2]
    N = CEM["population_size"]
    plain = _engine(L, U, opt=L.OPT_CEM, **CEM)                 # draws inside its rollout kernel
    twin = _engine(L, U, opt=L.OPT_CEM, **CEM)                  # the buffer form, nothing injected: shift_elites holds nothing at step 0
    twin.set_elite_carry(0, 1)
    eng = _engine(L, U, opt=L.OPT_CEM, **CEM)
    lr = 0.1 if method == "adam" else 2.0
    eng.set_grad_refine(2, lr, method, M)
    Nst, HU = 64, HQ * U                                        # population_size rounded up to the sample buffer's stride
    sentinel = np.full((2, HU, Nst), 123.0, F)
    for e in (plain, twin, eng):
        e.set_trace(True)
        e.set_state("sample_buffer", sentinel)
        e.optimize(states)
    # the padding columns n >= N: what the refined handle leaves there is what the twin leaves there
    raw, raw_twin = eng.get_state("sample_buffer", (2, HU, Nst)), twin.get_state("sample_buffer", (2, HU, Nst))
    np.testing.assert_array_equal(raw[:, :, N:], raw_twin[:, :, N:])
    np.testing.assert_array_equal(raw[:, :, N:], sentinel[:, :, N:])       # ... which is nothing: nobody writes them
    print("padding columns: sentinel kept in", int((raw[:, :, N:] == 123.0).sum()), "of", raw[:, :, N:].size, "elements (twin:",
          int((raw_twin[:, :, N:] == 123.0).sum()), ")")
    last = eng.get_trace(1, L.TRACE_SAMPLES)                     # the buffer's first N columns hold the last iteration's candidates
    np.testing.assert_array_equal(np.transpose(raw[:, :, :N], (2, 0, 1)).reshape(N, 2, HQ, U), last)
    base = twin.get_trace(0, L.TRACE_SAMPLES)                    # [N, A, H, U]
    np.testing.assert_array_equal(plain.get_trace(0, L.TRACE_SAMPLES), base)     # the twin can be relied on
    np.testing.assert_array_equal(plain.get_trace(0, L.TRACE_REWARDS), twin.get_trace(0, L.TRACE_REWARDS))
    got = eng.get_trace(0, L.TRACE_SAMPLES)
    m = M if M > 0 else N
    np.testing.assert_array_equal(got[:N - m], base[:N - m])
    helper = _engine(L, U)
    want = _columns_refined(L, helper, states, base[N - m:], 2, lr, method)
    np.testing.assert_array_equal(got[N - m:], want)
    assert np.any(got[N - m:] != base[N - m:])
    lo, hi = BOUNDS[U]
    assert np.all(got >= lo) and np.all(got <= hi)
    rewards = eng.get_trace(0, L.TRACE_REWARDS)                  # [N, A]
    np.testing.assert_allclose(rewards[N - m:], _model_returns(helper, U, states, got[N - m:]), rtol=R.H_STEP_RTOL,
                               atol=R.H_STEP_ATOL_PER_STEP * HQ)
    np.testing.assert_array_equal(rewards[:N - m], twin.get_trace(0, L.TRACE_REWARDS)[:N - m])
    assert np.all(np.isfinite(eng.get_trace(1, L.TRACE_SAMPLES)))


def test_switching_off_restores_the_bits(L, data):
    U = 1
    states = data[U][0][:2]
    a, b = _engine(L, U, opt=L.OPT_CEM, **CEM), _engine(L, U, opt=L.OPT_CEM, **CEM)
    a.set_trace(True)
    b.set_trace(True)
    a.set_grad_refine(2, 0.1)
    ra, rb = a.optimize(states, 0), b.optimize(states, 0)       # (b too: the draws are keyed by the handle's count of control steps)
    assert np.any(ra[0] != rb[0])
    a.set_grad_refine(0)
    assert a.get_grad_refine()[0] == 0
    a.reset()
    b.reset()
    for t in range(2):
        ra, rb = a.optimize(states, t), b.optimize(states, t)
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)
        for it in range(2):
            for item in (L.TRACE_SAMPLES, L.TRACE_REWARDS, L.TRACE_MEAN, L.TRACE_VAR):
                np.testing.assert_array_equal(a.get_trace(it, item), b.get_trace(it, item))


def test_composition_with_colored_noise_elite_carry_and_policy_prior(L, data):
    from blackbox_mpc_amd.utils.colored_noise import resolve_sampling_correlation
    U = 1
    states = data[U][0][:2]
    N, M = CEM["population_size"], 21
    rng = np.random.default_rng(5)
    pw = [rng.normal(0, 0.5, (3, 20)).astype(F), rng.normal(0, 0.5, (20, 1)).astype(F)]
    pb = [np.zeros(20, F), np.zeros(1, F)]

    def make(grad):
        e = _engine(L, U, opt=L.OPT_CEM, **CEM)
        e.set_sampling_correlation(resolve_sampling_correlation(HQ, 1.0, None))
        e.set_elite_carry(2, 2)
        e.set_policy_prior_mlp(pw, pb, [PG.ACT["tanh"], 0], count=3, noise_std=0.1)
        if grad:
            e.set_grad_refine(2, 0.1, "adam", M)
        e.set_trace(True)
        return e
    eng, twin, helper = make(True), make(False), _engine(L, U)
    # control step 0, iteration 0: nothing carried yet; the last columns hold the prior's rollouts
    eng.optimize(states, 0)
    twin.optimize(states, 0)
    base, got = twin.get_trace(0, L.TRACE_SAMPLES), eng.get_trace(0, L.TRACE_SAMPLES)
    np.testing.assert_array_equal(got[:N - M], base[:N - M])
    np.testing.assert_array_equal(got[N - M:], _columns_refined(L, helper, states, base[N - M:], 2, 0.1, "adam"))
    assert np.any(got[N - 3:] != base[N - 3:])                   # the prior's columns are refined too
    # control step 1: the carried (shifted) elites and the prior's columns are refined, everything stays finite
    out = eng.optimize(states, 1)
    assert all(np.all(np.isfinite(x)) for x in out)
    for it in range(2):
        assert np.all(np.isfinite(eng.get_trace(it, L.TRACE_SAMPLES))) and np.all(np.isfinite(eng.get_trace(it, L.TRACE_REWARDS)))
    lo, hi = BOUNDS[U]
    for it in range(2):                                          # the carried and the prior's columns stay inside the bounds
        tail = eng.get_trace(it, L.TRACE_SAMPLES)[N - M:]
        assert np.all(tail >= lo) and np.all(tail <= hi)


def test_composition_refines_the_carried_and_the_prior_columns(L, data):
    """M = keep + count = 5: exactly the carried elites and the policy's rollouts are refined, and both can be restated without
    a twin that shares the distribution: the carried columns are the handle's own sorted elites of the iteration before
    (k_elite_inject: elite e -> column N - count + e; across control steps moved one planning step forward, the last step
    repeated), the policy's columns are predict_policy_rollouts from the same state (noise_std = 0)."""
    from blackbox_mpc_amd.utils.colored_noise import resolve_sampling_correlation
    U, K, C = 1, 3, 2
    states = data[U][0][:2]
    N, M = CEM["population_size"], K + C
    rng = np.random.default_rng(5)
    pw = [rng.normal(0, 0.5, (3, 20)).astype(F), rng.normal(0, 0.5, (20, 1)).astype(F)]
    pb = [np.zeros(20, F), np.zeros(1, F)]
    eng = _engine(L, U, opt=L.OPT_CEM, **CEM)
    eng.set_sampling_correlation(resolve_sampling_correlation(HQ, 1.0, None))
    eng.set_elite_carry(C, C)
    eng.set_policy_prior_mlp(pw, pb, [PG.ACT["tanh"], 0], count=K, noise_std=0.0)
    eng.set_grad_refine(2, 0.1, "adam", M)
    eng.set_trace(True)
    helper = _engine(L, U)
    prior = eng.predict_policy_rollouts(states, want_states=False)[0]        # [K, A, H, U], clipped as the candidates are
    assert prior.shape == (K, 2, HQ, U)
    moved = 0

    def carried_from(samples, elites, shift):
        cols = np.stack([np.stack([samples[elites[a, e], a] for a in range(2)]) for e in range(C)])      # [C, A, H, U]
        return np.concatenate([cols[:, :, 1:], cols[:, :, -1:]], 2) if shift else cols

    eng.optimize(states, 0)
    s0, s1 = eng.get_trace(0, L.TRACE_SAMPLES), eng.get_trace(1, L.TRACE_SAMPLES)
    e0, e1 = eng.get_trace(0, L.TRACE_ELITES), eng.get_trace(1, L.TRACE_ELITES)
    # control step 0, iteration 0: nothing carried; the policy's rollouts sit in the last K columns
    np.testing.assert_array_equal(s0[N - K:], _columns_refined(L, helper, states, prior, 2, 0.1, "adam"))
    # iteration 1: [policy K | carried C]
    pre = np.concatenate([prior, carried_from(s0, e0, False)])
    want = _columns_refined(L, helper, states, pre, 2, 0.1, "adam")
    np.testing.assert_array_equal(s1[N - M:], want)
    moved += int(np.sum(want[K:] != pre[K:]))
    # control step 1, iteration 0: the shifted elites of the last iteration
    eng.optimize(states, 1)
    t0 = eng.get_trace(0, L.TRACE_SAMPLES)
    pre = np.concatenate([prior, carried_from(s1, e1, True)])
    want = _columns_refined(L, helper, states, pre, 2, 0.1, "adam")
    np.testing.assert_array_equal(t0[N - M:], want)
    moved += int(np.sum(want[K:] != pre[K:]))
    print("carried columns: elements the refinement moved:", moved)
    assert moved > 0                                             # (elites at a bound stay there: not all of them are)
    assert np.all(np.isfinite(t0)) and np.all(np.isfinite(eng.get_trace(1, L.TRACE_SAMPLES)))


# ---- 6. Python layers -----------------------------------------------------------------------------------------------------------
def _models(seed=0):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP
    act, obs = Box(low=[-2.0], high=[1.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    dyn = DeterministicMLP(layers=[4, 20, 3], activation_functions=["tanh", None], seed=seed)
    dyn.set_weights([w * s for w, s in zip(dyn.weights, (1.0, 0.1))], dyn.biases)       # small state changes
    handler = SystemDynamicsHandler(act, obs, dynamics_function=dyn, true_model=False, is_normalized=False)
    rew = LearnedRewardMLP(3, 1, [33, 1], ["tanh", None], inputs="sas", seed=seed + 1)
    return act, obs, handler, rew


def _policy(handler, rew, act, obs, A, **kw):
    from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy
    return MPCPolicy(reward_function=rew, env_action_space=act, env_observation_space=obs, dynamics_handler=handler, optimizer_name="CEM",
                     num_agents=A, planning_horizon=6, population_size=64, num_elite=8, max_iterations=3, seed=3, **kw)


def test_mpc_policy_with_grad_steps_runs_a_pendulum_episode(L):
    """the environment is the analytic pendulum; the policy plans through (untrained) learned networks of the pendulum's shapes"""
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    from blackbox_mpc_amd.utils.rollouts import ModelEnvironment, perform_rollouts
    _, obs, handler, rew = _models()
    act = Box(low=[-2.0], high=[2.0])
    handler = SystemDynamicsHandler(act, obs, dynamics_function=handler._dynamics_function, true_model=False, is_normalized=False)
    A, T = 2, 8
    theta = np.array([0.3, -2.0])
    start = np.stack([np.cos(theta), np.sin(theta), np.array([0.5, -0.5])], 1).astype(F)
    true_handler = SystemDynamicsHandler(act, obs, dynamics_function=PendulumTrueModel(), true_model=True)
    env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), start)
    pol = _policy(handler, rew, act, obs, A, grad_steps=2, grad_lr=0.05, grad_candidates=24)
    assert pol._optimizer._engine.get_grad_refine() == (2, F(0.05), "adam", 24)
    observations, actions, rewards = perform_rollouts(env, 1, T, pol)
    returns = np.sum(np.asarray(rewards[0]), axis=0)
    print("pendulum episode of %d steps, returns" % T, returns)
    assert returns.shape == (A,) and np.all(np.isfinite(returns)) and np.all(returns <= 0)
    acs = np.asarray(actions[0])
    assert np.all(np.isfinite(np.asarray(observations[0]))) and np.all(acs >= act.low) and np.all(acs <= act.high)


def test_mpc_policy_refine_device(L):
    from blackbox_mpc_amd.utils.plan_refinement import refine_plan
    act, obs, handler, rew = _models()
    A = 2
    dev = _policy(handler, rew, act, obs, A, refine_steps=3, refine_lr=0.05, refine_device=True)
    host = _policy(handler, rew, act, obs, A, refine_steps=3, refine_lr=0.05, refine_device=False)
    parent = _policy(handler, rew, act, obs, A, refine_steps=3, refine_lr=0.05)
    o = np.random.default_rng(1).normal(0, 0.5, (A, 3)).astype(F)
    rd, rh, rp = dev.act(o, 0), host.act(o, 0), parent.act(o, 0)
    for x, y in zip(rh, rp):
        np.testing.assert_array_equal(x, y)                      # refine_device=False keeps the host path's bits
    eng = dev._optimizer._engine
    np.testing.assert_array_equal(dev._unrefined_plan, host._unrefined_plan)
    want, want_r = eng.refine_plans(o, dev._unrefined_plan, 3, 0.05)
    np.testing.assert_array_equal(dev._refined_plan, want)      # acts on Engine.refine_plans of get_plan()
    np.testing.assert_array_equal(rd[0], want[:, 0])
    assert np.all(want_r >= eng.plan_gradient(o, dev._unrefined_plan)[0])
    # agreement with the host loop: 4 x the gap of the float32 chain to the float64 chain on the statement of these networks
    dn, rn = handler._dynamics_function, rew
    assert handler.normalization_stats() is None and rn.normalization_stats() is None

    class Net:
        def __init__(self, ws, bs, mask):
            self.ws, self.bs, self.acts, self.stats, self.mask, self.S, self.U = list(ws), list(bs), ["tanh", None], None, mask, 3, 1
    nets = (Net(dn.weights, dn.biases, 0), Net(rn.weights, rn.biases, rn.input_mask), None, 0.0)
    plan = dev._unrefined_plan
    lo, hi = np.asarray(act.low, F), np.asarray(act.high, F)
    x64, _ = PR.refine(lambda s, q: PG.value_and_grad(*nets, s, q), o, plan, 3, 0.05, lo, hi, "adam", keep=False)
    x32, _ = PR.refine(lambda s, q: PG.value_and_grad(*nets, s, q, dt=np.float32), o, plan, 3, F(0.05), lo, hi, "adam", keep=False,
                       dt=np.float32)
    tol = 4 * float(np.max(np.abs(x32 - x64)))
    gap = float(np.max(np.abs(dev._refined_plan.astype(np.float64) - host._refined_plan)))
    print("refine_device against the host loop: plan gap %.3g, tolerance %.3g" % (gap, tol))
    assert gap <= tol
