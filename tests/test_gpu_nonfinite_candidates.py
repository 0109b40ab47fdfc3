"""NaN candidates among ordinary ones, on every kernel that scores candidates ("Non-finite candidates").

The contract: a candidate whose reward sum is NaN scores exactly -1e6 (deterministic.py:75-77), and its non-finite values
never change another candidate's bits.  tests/nonfinite_util.py holds the poison patterns and the assertion;
tests/test_nonfinite_cpu.py shows that the NumPy oracle satisfies that assertion for every pattern and model used here.

(a) every learned-model rollout kernel (the table of tests/test_gpu_mlp_kernel_choice.py at N = 37, A = 2: two full
    16-tiles plus 5, nine quads plus 1),  (b) the one-step row kernels on either side of their 32-row switch,
(c) one case for every other family that scores candidates,  (d) a NaN start state for one of three agents through each of
the six optimizers.  NaN goes into action sequences, start states and row inputs only."""
import os

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import nonfinite_util as NF
from tests.nonfinite_util import STEP_NETS, gpu_shape, step_inputs
from tests.test_gpu_mlp_kernel_choice import CASES, _case, build_case, case_inputs

pytestmark = pytest.mark.gpu
F = np.float32
N, A = NF.GPU_N, NF.GPU_A


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in [k for k in os.environ if k.startswith("BBMPC_MLP_") or k == "BBMPC_USER_STEPWISE"]:
        monkeypatch.delenv(k)


def poison_and_check(evaluate, seq, what, expect=4):
    """evaluate(seq [N, A, H, U]) -> rewards [N, A]: the clean call, then every pattern against it"""
    clean = evaluate(seq)
    pats = NF.patterns(seq)
    assert len(pats) == expect
    for name, poisoned, hit in pats:
        NF.check(clean, evaluate(poisoned), hit, "%s %s" % (what, name))
    np.testing.assert_array_equal(evaluate(seq), clean)        # and the handle carries nothing over from a poisoned call
    return clean


# ---- (a) every learned-model rollout kernel ----------------------------------------------------------------------------
ROLLOUTS = [c for c in CASES if not c["step"]]


@pytest.mark.parametrize("case", ROLLOUTS, ids=[c["id"] for c in ROLLOUTS])
def test_learned_model_rollout_kernels(L, monkeypatch, case):
    c = gpu_shape(case)
    eng, _ = build_case(L, c, monkeypatch.setenv)
    states, seq = case_inputs(c)
    assert seq.shape == (N, A, case["H"], c["U"])
    poison_and_check(lambda s: eng.evaluate(states, s), seq, c["id"])
    assert eng.get_profile()[2] == c["name"]
    assert eng.profile_instantiation() == c["inst"]


# ---- (b) the one-step forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", STEP_NETS, ids=[n[0] for n in STEP_NETS])
@pytest.mark.parametrize("B", [9, 40])
def test_one_step_rows(L, monkeypatch, net, B):
    c = _case(net[0], net[1], net[2], None)
    eng, ev = build_case(L, c, monkeypatch.setenv)
    s, a = step_inputs(c, B)
    nxt = eng.predict_next_state(s, a)
    nxt_o = ev.predict_next_state(s, a)                        # the reward rows take the oracle's next states, as everywhere
    rew = eng.evaluate_next_reward(s, nxt_o, a)
    for row in (0, B - 1):
        ap = a.copy()
        ap[row, -1] = np.nan
        with np.errstate(all="ignore"):
            want_n = ev.predict_next_state(s, ap)[[row]]
            want_r = ev.evaluate_next_reward(s, nxt_o, ap)[[row]]
        assert np.all(np.isnan(want_n))
        NF.check_rows(nxt, eng.predict_next_state(s, ap), want_n, [row], "%s next state, row %d of %d" % (net[0], row, B))
        got_r = eng.evaluate_next_reward(s, nxt_o, ap)
        if np.isnan(want_r[0]):
            want = want_r
        else:                                                  # a reward that does not read the action: the clean row's own bits
            np.testing.assert_allclose(rew[[row]], want_r, rtol=1e-5, atol=1e-4)
            want = rew[[row]]
        NF.check_rows(rew, got_r, want, [row], "%s reward, row %d of %d" % (net[0], row, B))


@pytest.mark.parametrize("net", STEP_NETS, ids=[n[0] for n in STEP_NETS])
def test_one_step_row_kernels_switch_between_32_and_33_rows(L, monkeypatch, net):
    """Which kernel serves 9 rows and which 40.  The one-step calls report no kernel name (the engine switches profiling off
    around them), so the switch is pinned by its arithmetic: up to 32 rows a workgroup per row on plain FMAs (k_rows_mlp), from
    33 on the one-step form of the MFMA rollout, which sums in another order.  Rows are independent, so within one kernel a
    prefix of the rows gives the same bits whatever the batch; across the switch the bits differ."""
    c = _case(net[0], net[1], net[2], None)
    eng, _ = build_case(L, c, monkeypatch.setenv)
    s, a = step_inputs(c, 40)
    out = {B: eng.predict_next_state(s[:B], a[:B]) for B in (9, 32, 33, 40)}
    np.testing.assert_array_equal(out[9].view(np.uint32), out[32][:9].view(np.uint32))
    np.testing.assert_array_equal(out[33].view(np.uint32), out[40][:33].view(np.uint32))
    assert not np.array_equal(out[32].view(np.uint32), out[33][:32].view(np.uint32))
    np.testing.assert_allclose(out[32], out[33][:32], rtol=2e-5, atol=2e-5)


# ---- (c) every other family that scores candidates ------------------------------------------------------------------------
def _seq(H, U, lim=1.0, seed=9):
    return np.random.default_rng(seed + H + U).uniform(-lim, lim, (N, A, H, U)).astype(F)


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_analytic_pendulum(L, strict):
    from blackbox_mpc_amd.engine import Engine
    H = 7
    eng = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H,
                 quirks=L.STRICT_MATH if strict else 0)
    states = O.pendulum_start_states(A)
    poison_and_check(lambda s: eng.evaluate(states, s), _seq(H, 1, 2.0), "k_rollout_pendulum")


@pytest.mark.parametrize("form", ["fused", "stepwise"])
@pytest.mark.parametrize("which", ["reward", "dynamics", "both"])
def test_hip_source_dynamics_and_reward(L, monkeypatch, form, which):
    from blackbox_mpc_amd.engine import Engine
    from tests.test_gpu_user_functions import INTENDED_PENDULUM_REWARD, USER_PENDULUM_MODEL
    if form == "stepwise":
        monkeypatch.setenv("BBMPC_USER_STEPWISE", "1")
    H = 7
    eng = Engine(L.OPT_NONE, L.DYN_PENDULUM if which == "reward" else L.DYN_USER,
                 L.REW_PENDULUM if which == "dynamics" else L.REW_USER, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H)
    if which != "reward":
        eng.set_dynamics_source(USER_PENDULUM_MODEL)
    if which != "dynamics":
        eng.set_reward_source(INTENDED_PENDULUM_REWARD)
    states = O.pendulum_start_states(A)
    poison_and_check(lambda s: eng.evaluate(states, s), _seq(H, 1, 2.0), "user functions %s %s" % (form, which))


@pytest.mark.parametrize("form", ["fused", "stepwise"])
@pytest.mark.parametrize("net,xform", [("cheetah", "scaled"), ("pendulum", "wrap")])
def test_target_transform_rollout(L, monkeypatch, form, net, xform):
    from tests import test_gpu_target_transforms as T
    if form == "stepwise":
        monkeypatch.setenv("BBMPC_USER_STEPWISE", "1")
    H = 5
    eng, spec = T._engine(L, net, L.REW_PENDULUM if net == "pendulum" else L.REW_USER, xform, A, H, True)
    S, U = spec[4], spec[5]
    states = T._start(S, A)
    poison_and_check(lambda s: eng.evaluate(states, s), _seq(H, U), "transform %s %s %s" % (form, net, xform))


def test_reward_mlp_trajectory_scorer(L):
    from tests import reward_mlp_util as R
    from tests import test_gpu_reward_mlp as G
    for net, H in [(R.small_nets()[1], 5), (R.small_nets()[4], 5), (R.medium_net(), 4)]:
        eng = G._engine(L, net, A=A, H=H, hidden=[200, 200] if net.S == 20 else None)
        states = G._states(net, A)
        poison_and_check(lambda s: eng.evaluate(states, s), _seq(H, net.U), "reward MLP " + net.name)


@pytest.mark.parametrize("kind", ["builtin", "user", "mlp"])
def test_terminal_value_finish(L, kind):
    from tests import terminal_value_util as V
    from tests import test_gpu_terminal_value as G
    H = 5
    eng = G._engine(L, kind, A=A, H=H)
    G._set(eng, V.small_nets()[1], -0.5)
    states = G._states(A)
    poison_and_check(lambda s: eng.evaluate(states, s), _seq(H, 1), "terminal value over a %s reward" % kind)


def check_particles(eng, states, seq, P, what):
    """The particle evaluator: a poisoned candidate scores -1e6 with all its particle returns -1e6; every other candidate's
    score and returns are the clean call's bits."""
    s0, r0 = eng.evaluate_particles(states, seq)
    assert r0.shape == (N, P, A) and not np.isnan(r0).any()
    for name, poisoned, hit in NF.patterns(seq):
        s1, r1 = eng.evaluate_particles(states, poisoned)
        NF.check(s0, s1, hit, "%s %s: scores" % (what, name))
        for p in range(P):
            NF.check(np.ascontiguousarray(r0[:, p]), np.ascontiguousarray(r1[:, p]), hit, "%s %s: returns of particle %d" % (what, name, p))


def test_particle_evaluator_analytic_pendulum(L):
    from tests.test_gpu_particles import _engine
    from tests.test_particles_cpu import PEND_SIGMA
    P, H = 3, 7
    eng = _engine(L, L.OPT_NONE, A, H)
    eng.set_particles(P, PEND_SIGMA, 1.5)
    eng.inject_noise(L.NOISE_PROCESS, np.random.default_rng(3).standard_normal((A, P, H, 3)).astype(F))
    check_particles(eng, O.pendulum_start_states(A), _seq(H, 1, 2.0), P, "pendulum particles")


@pytest.mark.parametrize("net", ["cheetah", "pendulum"])
@pytest.mark.parametrize("members", [1, 2], ids=["one_model", "ensemble"])
def test_particle_evaluator_learned_model(L, net, members):
    from tests.test_ensemble_cpu import member_evaluators, network
    from tests.test_gpu_ensemble import _engine
    spec = network("CHEETAH" if net == "cheetah" else "PEND_MLP")
    S, U = spec[2], spec[3]
    P, H = 4, 5
    params, stats, _ = member_evaluators(spec, 2)
    eng = _engine(L, spec, params, stats, A, H)
    eng.set_particles(P, np.full(S, 0.02, F), 1.5)
    if members > 1:
        eng.set_mlp_ensemble(params)
    eng.inject_noise(L.NOISE_PROCESS, np.random.default_rng(4).standard_normal((A, P, H, S)).astype(F))
    states = O.cheetah_start_states(A, S) if net == "cheetah" else O.pendulum_start_states(A)
    eng.set_profiling(True)
    check_particles(eng, states, _seq(H, U), P, "%s particles, %d model(s)" % (net, members))
    assert eng.get_profile()[2] == ("k_rollout_mlp_particles_ens" if members > 1 else "k_rollout_mlp_particles")


def test_particle_evaluator_with_hip_source_reward(L):
    from tests.test_ensemble_cpu import member_evaluators, network
    from tests.test_gpu_mlp import Q4S_USER_REWARD
    from blackbox_mpc_amd.engine import Engine
    from tests.test_gpu_activations import CODE
    spec = network("PEND_MLP")
    dims, acts, S, U, _ = spec
    P, H = 4, 5
    params, stats, _ = member_evaluators(spec, 1)
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_USER, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=A, planning_horizon=H)
    eng.set_reward_source(Q4S_USER_REWARD)
    eng.set_mlp(params[0][0], params[0][1], [CODE[a] for a in acts], stats)
    eng.set_particles(P, np.full(S, 0.02, F), 1.5)
    eng.inject_noise(L.NOISE_PROCESS, np.random.default_rng(5).standard_normal((A, P, H, S)).astype(F))
    check_particles(eng, O.pendulum_start_states(A), _seq(H, U), P, "particles with a HIP-source reward")


# ---- (d) a NaN start state for one of three agents, through each optimizer -------------------------------------------------
OPTS = ["RandomSearch", "CEM", "PI2", "PSO", "CMA-ES", "SPSA"]
MODELS = {"pendulum": ([4, 32, 32, 32, 3], ["tanh", "tanh", "tanh", None], 3, 1, "pendulum", "k_rollout_mlp_w4"),
          "cheetah": ([26, 200, 200, 20], ["tanh", "tanh", None], 20, 6, "cheetah", "k_rollout_mlp_q4s"),
          # the analytic pendulum: the persistent control-step kernels, and for CMA-ES with the trace on the per-iteration
          # rollout (test_cmaes_untraced_kernels_on_the_analytic_pendulum runs its other two)
          "analytic": (None, None, 3, 1, "pendulum",
                       {"RandomSearch": "k_fused_pendulum", "CEM": "k_fused_pendulum", "PI2": "k_fused_pendulum",
                        "SPSA": "k_fused_pendulum", "PSO": "k_fused_pso_pendulum", "CMA-ES": "k_rollout_pendulum"})}


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("opt_name", OPTS)
def test_nan_start_state_of_one_agent_in_the_optimizers(L, opt_name, model):
    """CMA-ES runs in its per-agent mode: the reference's coupled mode sums the rewards over the agents (cma_es.py:158), so
    there the agents are one candidate and a NaN agent is part of every one of them.  Its draws alone are injected: finite
    normal draws small enough that no candidate leaves the action bounds (nonfinite_util.bounded_normal_draws), because the
    reference subtracts the bound penalty from the evaluator's -1e6 (cma_es.py:149-157) and the engine's own unit normal
    draws at sigma = range / 4 leave the bounds (measured -1000000.06 .. -1000001).  The traced samples are the clipped
    candidates, so the penalty cannot be recomputed from them.  They are read for CEM and PI2 only."""
    from tests.test_gpu_mlp import _problem
    dims, acts, S, U, reward, kernel = MODELS[model]
    if isinstance(kernel, dict):
        kernel = kernel[opt_name]
    Np, Ag, H, iters, k, alpha = 96, 3, 6, 2, 12, 0.25
    opt = {"RandomSearch": L.OPT_RANDOM_SEARCH, "CEM": L.OPT_CEM, "PI2": L.OPT_PI2, "PSO": L.OPT_PSO, "CMA-ES": L.OPT_CMAES,
           "SPSA": L.OPT_SPSA}[opt_name]
    kw = dict(quirks=L.CMAES_PER_AGENT) if opt_name == "CMA-ES" else {}
    clean_states = (O.cheetah_start_states(Ag, S) if reward == "cheetah" else O.pendulum_start_states(Ag)).astype(F)
    bad_states = clean_states.copy()
    bad_states[1, S - 1] = np.nan
    out = []
    for states in (bad_states, clean_states):
        its = 0 if opt_name == "RandomSearch" else iters
        if dims is None:
            from blackbox_mpc_amd.engine import Engine
            lo, hi = [-2.0], [2.0]
            eng = Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, lo, hi, dim_s=3, num_agents=Ag, planning_horizon=H,
                         population_size=Np, max_iterations=its, num_elite=k, alpha=alpha, **kw)
        else:
            eng, _, lo, hi = _problem(L, dims, acts, S, U, reward, True, A=Ag, H=H, opt=opt, N=Np, iters=its, k=k, alpha=alpha, **kw)
        eng.set_trace(True)
        eng.set_profiling(True)
        eng.reset()
        if opt_name == "CMA-ES":
            eng.inject_noise(L.NOISE_NORMAL, NF.bounded_normal_draws(np.random.default_rng(11), (iters, Np, Ag, H, U)))
        act, nxt, rew = eng.optimize(states)
        assert eng.get_profile()[2] == kernel
        tr = [(eng.get_trace(it, L.TRACE_REWARDS), eng.get_trace(it, L.TRACE_SAMPLES)) for it in range(eng.iters)]
        elites = [eng.get_trace(it, L.TRACE_ELITES) for it in range(eng.iters)] if opt_name == "CEM" else None
        out.append((act, nxt, rew, tr, elites))
    (act, nxt, rew, tr, elites), (act_c, nxt_c, rew_c, tr_c, _) = out
    assert len(tr) == (1 if opt_name == "RandomSearch" else iters)
    for it, ((r, x), (r_c, x_c)) in enumerate(zip(tr, tr_c)):
        print("[%s %s] iteration %d: agent 1's distinct traced rewards %s" % (opt_name, model, it, np.unique(r[:, 1])[:4]))
        assert np.all(r[:, 1] == F(-1e6)), (it, np.unique(r[:, 1])[:8])
        assert not np.isnan(r_c).any() and not (r_c <= F(-1e6)).any()
        for a in (0, 2):
            np.testing.assert_array_equal(r[:, a].view(np.uint32), r_c[:, a].view(np.uint32))
    for a in (0, 2):
        for got, want in ((act, act_c), (nxt, nxt_c), (rew, rew_c)):
            np.testing.assert_array_equal(np.ascontiguousarray(got[a]).view(np.uint32), np.ascontiguousarray(want[a]).view(np.uint32))
    assert np.all(np.isfinite(act[1])) and np.all(act[1] >= np.asarray(lo, F)) and np.all(act[1] <= np.asarray(hi, F))
    if opt_name == "CEM":
        # every reward ties at -1e6: top_k takes the lower index first, so the elites are samples 0 .. k-1 (cem.py:97-122)
        mean = np.zeros((H, U))                                # the bounds' midpoint
        for it in range(iters):
            np.testing.assert_array_equal(np.sort(elites[it][1]), np.arange(k))
            mean = alpha * mean + (1.0 - alpha) * tr[it][1][:k, 1].astype(np.float64).mean(axis=0)
        np.testing.assert_allclose(act[1], mean[0], rtol=0, atol=1e-4)
    if opt_name == "PI2":
        # equal costs, equal weights 1 / N (pi2.py:78-87): the plain average of the last iteration's samples
        np.testing.assert_allclose(act[1], tr[-1][1][:, 1, 0].astype(np.float64).mean(axis=0), rtol=0, atol=2e-5)


@pytest.mark.parametrize("fused", [False, True], ids=["k_cma_sample_roll_small", "k_fused_cma_pendulum"])
def test_cmaes_untraced_kernels_on_the_analytic_pendulum(L, monkeypatch, fused):
    """Per-agent CMA-ES on the analytic pendulum with the trace off: by default the rollouts ride on the sampling launch
    (k_cma_sample_roll_small), with BBMPC_CMA_FUSED=1 the whole control step is one launch (k_fused_cma_pendulum).  Both
    hold the -1e6 rule for their own rollouts; without a trace the statement is the agents': a NaN start state for agent 1
    of 3 leaves agents 0 and 2 their bits and agent 1 a finite action inside the bounds.  Engine-drawn noise."""
    from blackbox_mpc_amd.engine import Engine
    monkeypatch.delenv("BBMPC_FUSED", raising=False)
    if fused:
        monkeypatch.setenv("BBMPC_CMA_FUSED", "1")
    else:
        monkeypatch.delenv("BBMPC_CMA_FUSED", raising=False)
    Np, Ag, H, iters, k = 96, 3, 6, 2, 12
    lo, hi = [-2.0], [2.0]
    clean_states = O.pendulum_start_states(Ag).astype(F)
    bad_states = clean_states.copy()
    bad_states[1, 2] = np.nan
    out = []
    for states in (bad_states, clean_states):
        eng = Engine(L.OPT_CMAES, L.DYN_PENDULUM, L.REW_PENDULUM, lo, hi, dim_s=3, num_agents=Ag, planning_horizon=H,
                     population_size=Np, max_iterations=iters, num_elite=k, quirks=L.CMAES_PER_AGENT)
        eng.set_profiling(True)
        eng.reset()
        steps = [eng.optimize(states) for _ in range(2)]       # the second control step starts from the first one's state
        assert eng.get_profile()[2] == ("k_fused_cma_pendulum" if fused else "k_cma_sample_roll_small")
        out.append(steps)
    for (act, nxt, rew), (act_c, nxt_c, rew_c) in zip(*out):
        assert np.all(np.isfinite(act_c)) and np.all(np.isfinite(nxt_c)) and np.all(np.isfinite(rew_c))
        for a in (0, 2):
            for got, want in ((act, act_c), (nxt, nxt_c), (rew, rew_c)):
                np.testing.assert_array_equal(np.ascontiguousarray(got[a]).view(np.uint32), np.ascontiguousarray(want[a]).view(np.uint32))
        assert np.all(np.isfinite(act[1])) and np.all(act[1] >= np.asarray(lo, F)) and np.all(act[1] <= np.asarray(hi, F))
