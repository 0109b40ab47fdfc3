"""GPU tests of the host-in / host-out wrappers of the C ABI, which all stage through one buffer per handle (csrc/abi_util.hpp
HostStage).  Everything is compared bit for bit (np.array_equal on the float32 views):

1. host == device: every wrapper with a _dev twin returns what the twin writes into torch tensors;
2. order independence: every wrapper at the small sizes, then every wrapper at the large size in a shuffled order (the
   shared buffer grows under each in turn), then the small sizes again in another order -- the third round is the first;
3. optional outputs: a call without one of its outputs gives the others unchanged;
4. a refused call between two equal good ones changes nothing.

Shapes: S = 3, U = 1, hidden [24], A = 2, H = 3; batch / n_pop 1, 5 and 70 (70 crosses the 32-row switch of the one-step
kernels and the 64-row tile).  Handles as the mutual exclusions force them: "M" DYN_MLP + REW_MLP + terminal value (plan
gradient, refinement), "C" CEM + policy prior, "P" particles (no value network), "S" PSO on the analytic pendulum (the
scalar draws of dump_noise)."""
import ctypes

import numpy as np
import pytest

from tests import policy_prior_util as PP
from tests import terminal_value_util as V
from tests.test_gpu_terminal_value import _engine, _dynamics

pytestmark = pytest.mark.gpu
F = np.float32
S, U, A, H = 3, 1, 2, 3
K_PRIOR, P_PART, N_CEM = 5, 4, 64
SMALL, LARGE = (1, 5), 70
FWD_XFORM = ("__device__ void bbmpc_user_transform_targets(const float* cur, const float* next, float* t, int S) {\n"
             "    for (int i = 0; i < S; ++i) t[i] = 2.0f * (next[i] - cur[i]);\n}\n")


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _handles(L, xform=False):
    """xform: "M" also gets a forward target transform (one run-time compilation), for bbmpc_transform_rows"""
    from blackbox_mpc_amd.engine import Engine
    m = _engine(L, "mlp", A=A, H=H)
    vnet = V.small_nets()[1]
    m.set_terminal_value_mlp(vnet.ws, vnet.bs, vnet.codes(), vnet.stats, 0.5)
    if xform:
        m.set_transform_source(FWD_XFORM)
    c = _engine(L, "builtin", A=A, H=H, opt=L.OPT_CEM, population_size=N_CEM, max_iterations=2, num_elite=8)
    PP.small_policies(S, U)[1].install(c, K_PRIOR, 0.2)
    rng = np.random.default_rng(3)                             # injected draws: every control step sees the same ones (_episode)
    c.inject_noise(L.NOISE_TRUNC_NORMAL, np.clip(rng.normal(size=(2, N_CEM, A, H, U)), -2, 2).astype(F))
    c.inject_noise(L.NOISE_POLICY, rng.normal(size=(2, A, K_PRIOR, H, U)).astype(F))
    p = _engine(L, "builtin", A=A, H=H)
    p.set_particles(P_PART, [0.05, 0.02, 0.1], 0.5)
    s = Engine(L.OPT_PSO, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=S, num_agents=A, planning_horizon=H,
               population_size=N_CEM, max_iterations=2)
    return {"M": m, "C": c, "P": p, "S": s}


@pytest.fixture(scope="module")
def hd(L):
    return _handles(L)


def _draw(idx, b, *shapes, lo=-1.0, hi=1.0):
    """the inputs of wrapper `idx` at size b: the same whenever they are asked for"""
    rng = np.random.default_rng([idx, b])
    return [rng.uniform(lo, hi, sh).astype(F) for sh in shapes]


def _tup(x):
    return tuple(v for v in (x if isinstance(x, (tuple, list)) else (x,)) if v is not None)


# name -> (handle, index for the inputs, call(engine, L, b) -> arrays).  Every host-in / host-out wrapper is here.
def _evaluate(e, L, b):
    return e.evaluate(*_draw(0, b, (A, S), (b, A, H, U)))


def _predict_trajectories(e, L, b):
    return e.predict_trajectories(*_draw(1, b, (b, S), (b, H, U)))


def _terminal_value(e, L, b):
    return e.evaluate_terminal_value(*_draw(2, b, (b, S)))


def _plan_gradient(e, L, b):
    return e.plan_gradient(*_draw(3, b, (b, S), (b, H, U)))


def _refine_plans(e, L, b):
    return e.refine_plans(*_draw(4, b, (b, S), (b, H, U)), 2, 0.1, "adam", True)


def _next_state(e, L, b):
    return e.predict_next_state(*_draw(5, b, (b, S), (b, U)))


def _next_reward(e, L, b):
    return e.evaluate_next_reward(*_draw(6, b, (b, S), (b, S), (b, U)))


def _process_input(e, L, b):
    return e.process_input(*_draw(7, b, (b, S), (b, U)), stats=_dynamics(S, U, [24])[3])


def _process_output(e, L, b):
    return e.process_output(*_draw(8, b, (b, S), (b, S)))


def _transform_rows(e, L, b):
    return e.transform_rows(L.USER_KIND_TRANSFORM, *_draw(9, b, (b, S), (b, S)))


def _mlp_forward(e, L, b):
    return e.mlp_forward(*_draw(10, b, (b, S + U)))


def _policy_rows(e, L, b):
    return e.evaluate_policy_prior(*_draw(11, b, (b, S)))


def _policy_rollouts(e, L, b):
    st, nz = _draw(12, b, (A, S), (A, K_PRIOR, H, U))
    return e.predict_policy_rollouts(st, nz)


def _episode(e, L, b):
    e.reset()                                                  # the distribution starts over; the draws are the injected ones
    return e.rollout_episode(_draw(13, b, (A, S))[0], 1 if b < LARGE else 3)


def _dump_samples(e, L, b):
    return e.dump_noise(L.NOISE_TRUNC_NORMAL, 1, 0, (N_CEM, A, H, U))


def _dump_policy(e, L, b):
    return e.dump_noise(L.NOISE_POLICY, 1, 0, (A, K_PRIOR, H, U))


def _particles(e, L, b):
    return e.evaluate_particles(*_draw(14, b, (A, S), (b, A, H, U)))


def _traj_particles(e, L, b):
    st, seq, eps = _draw(15, b, (b, S), (b, H, U), (b, P_PART, H, S))
    return e.predict_trajectory_particles(st, seq, eps, want_particles=True)


def _traj_quantiles(e, L, b):
    st, seq, eps = _draw(16, b, (b, S), (b, H, U), (b, P_PART, H, S))
    return e.predict_trajectory_particles(st, seq, eps, want_particles=True, quantile_ranks=[0, 2])


def _dump_process(e, L, b):
    return e.dump_noise(L.NOISE_PROCESS, 1, 0, (A, P_PART, H, S))


def _dump_scalars(e, L, b):
    return e.dump_noise(L.NOISE_PSO_SCALARS, 1, 0, (2,))


def _dump_exploration(e, L, b):
    return e.dump_noise(L.NOISE_EXPLORATION, 1, 0, (A, U))


WRAPPERS = [("M", _evaluate), ("M", _predict_trajectories), ("M", _terminal_value), ("M", _plan_gradient), ("M", _refine_plans),
            ("M", _next_state), ("M", _next_reward), ("M", _process_input), ("M", _process_output), ("M", _transform_rows),
            ("M", _mlp_forward), ("C", _policy_rows), ("C", _policy_rollouts), ("C", _episode), ("C", _dump_samples),
            ("C", _dump_policy), ("P", _particles), ("P", _traj_particles), ("P", _traj_quantiles), ("P", _dump_process),
            ("S", _dump_scalars), ("S", _dump_exploration)]


def _same(got, want, what):
    got, want = _tup(got), _tup(want)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, i)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), "%s: output %d differs" % (what, i)


# ---- 1. host == device -------------------------------------------------------------------------------------------------------
def _dev_twin(torch, eng, inputs, out_shapes, call):
    """inputs / outputs as torch tensors on the handle's device; call(pointers of the inputs, pointers of the outputs)"""
    dev = torch.device("cuda", eng.device)
    d_in = [torch.from_numpy(np.ascontiguousarray(v, F)).to(dev) for v in inputs]
    d_out = [torch.full(sh, float("nan"), device=dev) for sh in out_shapes]
    torch.cuda.synchronize(dev)
    call([t.data_ptr() for t in d_in], [t.data_ptr() for t in d_out])
    eng.synchronize()
    return tuple(t.cpu().numpy() for t in d_out)


@pytest.mark.parametrize("b", SMALL + (LARGE,))
def test_host_form_equals_the_dev_form(L, hd, b):
    import torch
    m, c, p = hd["M"], hd["C"], hd["P"]
    ins = _draw(0, b, (A, S), (b, A, H, U))
    _same(m.evaluate(*ins), _dev_twin(torch, m, ins, [(b, A)], lambda i, o: m.evaluate_dev(i[0], i[1], b, o[0])), "evaluate")
    ins = _draw(1, b, (b, S), (b, H, U))
    _same(m.predict_trajectories(*ins),
          _dev_twin(torch, m, ins, [(b, H, S), (b, H)], lambda i, o: m.predict_trajectories_dev(i[0], i[1], b, H, o[0], o[1])),
          "predict_trajectories")
    ins = _draw(2, b, (b, S))
    _same(m.evaluate_terminal_value(*ins), _dev_twin(torch, m, ins, [(b,)], lambda i, o: m.evaluate_terminal_value_dev(i[0], b, o[0])),
          "evaluate_terminal_value")
    ins = _draw(3, b, (b, S), (b, H, U))
    _same(m.plan_gradient(*ins),
          _dev_twin(torch, m, ins, [(b,), (b, H, U)], lambda i, o: m.plan_gradient_dev(i[0], i[1], b, H, o[0], o[1])), "plan_gradient")
    ins = _draw(4, b, (b, S), (b, H, U))
    plans, rets = m.refine_plans(*ins, 2, 0.1, "adam", True)
    dev = torch.device("cuda", m.device)                       # (the plans are refined in place: read the input tensor back)
    d_s, d_q = torch.from_numpy(ins[0]).to(dev), torch.from_numpy(ins[1]).to(dev)
    d_r = torch.full((b,), float("nan"), device=dev)
    torch.cuda.synchronize(dev)
    m.refine_plans_dev(d_s.data_ptr(), d_q.data_ptr(), b, H, 2, 0.1, "adam", True, d_r.data_ptr())
    m.synchronize()
    _same((plans, rets), (d_q.cpu().numpy(), d_r.cpu().numpy()), "refine_plans")
    assert not np.array_equal(plans, ins[1])                   # (the steps moved the plans)

    ins = _draw(11, b, (b, S))
    _same(c.evaluate_policy_prior(*ins), _dev_twin(torch, c, ins, [(b, U)], lambda i, o: c.evaluate_policy_prior_dev(i[0], b, o[0])),
          "evaluate_policy_prior")
    ins = _draw(12, b, (A, S), (A, K_PRIOR, H, U))
    _same(c.predict_policy_rollouts(*ins),
          _dev_twin(torch, c, ins, [(K_PRIOR, A, H, U), (K_PRIOR, A, H, S)], lambda i, o: c.predict_policy_rollouts_dev(i[0], i[1], o[0], o[1])),
          "predict_policy_rollouts")

    ins = _draw(14, b, (A, S), (b, A, H, U))
    _same(p.evaluate_particles(*ins),
          _dev_twin(torch, p, ins, [(b, A), (b, P_PART, A)], lambda i, o: p.evaluate_particles_dev(i[0], i[1], b, o[0], o[1])),
          "evaluate_particles")
    ins = _draw(15, b, (b, S), (b, H, U), (b, P_PART, H, S))
    moments = [(b, H, S), (b, H, S), (b, H), (b, H)]
    parts = [(b, P_PART, H, S), (b, P_PART, H)]
    _same(p.predict_trajectory_particles(*ins, want_particles=True),
          _dev_twin(torch, p, ins, moments + parts, lambda i, o: p.predict_trajectory_particles_dev(i[0], i[1], b, H, i[2], *o)),
          "predict_trajectory_particles")
    quants = [(b, 2, H, S), (b, 2, H)]
    _same(p.predict_trajectory_particles(*ins, want_particles=True, quantile_ranks=[0, 2]),      # (moments, quantiles, particles)
          _dev_twin(torch, p, ins, moments + quants + parts,
                    lambda i, o: p.predict_trajectory_quantiles_dev(i[0], i[1], b, H, [0, 2], i[2], o[0], o[1], o[2], o[3], o[6], o[7], o[4], o[5])),
          "predict_trajectory_quantiles")


# ---- 2. order independence ---------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_ran_before(L):
    hd = _handles(L, xform=True)                               # fresh: the first large call of a handle grows its buffer
    names = list(range(len(WRAPPERS)))

    def run(i, b):
        h, fn = WRAPPERS[i]
        return _tup(fn(hd[h], L, b))
    first = {(i, b): run(i, b) for b in SMALL for i in names}
    order = list(np.random.default_rng(7).permutation(names))
    large = {i: run(i, LARGE) for i in order}
    for i in names:                                            # (the large results are results: finite, and not the small ones)
        assert all(np.all(np.isfinite(v)) for v in large[i]), WRAPPERS[i][1].__name__
    other = list(np.random.default_rng(8).permutation(names))
    assert other != order and other != names
    for b in reversed(SMALL):
        for i in other:
            _same(run(i, b), first[(i, b)], "%s at %d after the large round" % (WRAPPERS[i][1].__name__, b))
    for i in order[::-1]:                                      # and the large size once more, after the small ones
        _same(run(i, LARGE), large[i], "%s at %d, second time" % (WRAPPERS[i][1].__name__, LARGE))


# ---- 3. optional outputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", SMALL + (LARGE,))
def test_an_output_that_is_not_wanted_changes_no_other(L, hd, b):
    m, p = hd["M"], hd["P"]
    ins = _draw(1, b, (b, S), (b, H, U))
    both = m.predict_trajectories(*ins)
    only_s, none_r = m.predict_trajectories(*ins, want_rewards=False)
    none_s, only_r = m.predict_trajectories(*ins, want_states=False)
    assert none_r is None and none_s is None
    _same(only_s, both[0], "predict_trajectories, states only")
    _same(only_r, both[1], "predict_trajectories, rewards only")
    ins = _draw(3, b, (b, S), (b, H, U))
    ret, grad = m.plan_gradient(*ins)
    none_ret, grad2 = m.plan_gradient(*ins, want_returns=False)
    assert none_ret is None and ret.shape == (b,)
    _same(grad2, grad, "plan_gradient without returns_out")
    ins = _draw(14, b, (A, S), (b, A, H, U))
    scores, returns = p.evaluate_particles(*ins)
    scores2, none_returns = p.evaluate_particles(*ins, want_returns=False)
    assert none_returns is None and returns.shape == (b, P_PART, A)
    _same(scores2, scores, "evaluate_particles without returns")


# ---- 4. a refusal in between -------------------------------------------------------------------------------------------------
def test_a_refused_call_between_two_good_ones(L, hd):
    m, p = hd["M"], hd["P"]
    b = 5
    z = np.zeros((1, 4), F)                                    # (batch 0 reads none of it)
    out = np.full((b, H, S), 7.0, F)

    def refused(code, text):
        assert code == L.E_INVALID
        assert L.lib.bbmpc_last_error().decode() == text

    for fn, bad, text in [
            (_next_state, lambda: L.lib.bbmpc_predict_next_state(m._h, L.ptr(z), L.ptr(z), 0, L.ptr(out)), "batch must be >= 1"),
            (_predict_trajectories, lambda: L.lib.bbmpc_predict_trajectories(m._h, L.ptr(z), L.ptr(z), 0, H, L.ptr(out), None), "batch must be >= 1"),
            (_terminal_value, lambda: L.lib.bbmpc_evaluate_terminal_value(m._h, L.ptr(z), 0, L.ptr(out)), "batch must be >= 1"),
            (_process_input, lambda: L.lib.bbmpc_process_input(m._h, L.ptr(z), L.ptr(z), 0, None, L.ptr(out)), "batch must be >= 1"),
            (_mlp_forward, lambda: L.lib.bbmpc_mlp_forward(m._h, L.ptr(z), 0, L.ptr(out)), "batch must be >= 1"),
            (_evaluate, lambda: L.lib.bbmpc_evaluate(m._h, L.ptr(out), L.ptr(z), 0, L.ptr(out)), "n_pop must be >= 1")]:
        before = fn(m, L, b)
        refused(bad(), text)
        assert np.all(out == 7.0)                              # nothing was written
        _same(fn(m, L, b), before, fn.__name__)
    before = _particles(p, L, b)
    refused(L.lib.bbmpc_evaluate_particles(p._h, L.ptr(out), L.ptr(z), 0, L.ptr(out), None), "n_pop must be >= 1")
    _same(_particles(p, L, b), before, "evaluate_particles")
    # a null statistics vector is refused before the staging buffer is touched, too
    before = _process_input(m, L, b)
    st = _dynamics(S, U, [24])[3]
    sp = (ctypes.c_void_p * 6)(*[v.ctypes.data for v in st[:5]], None)
    a, u = _draw(7, b, (b, S), (b, U))
    refused(L.lib.bbmpc_process_input(m._h, L.ptr(a), L.ptr(u), b, sp, L.ptr(out)), "null statistics vector")
    assert np.all(out == 7.0)
    _same(_process_input(m, L, b), before, "process_input")
