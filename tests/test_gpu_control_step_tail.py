"""The tail of every control step (optimizer_base.py:82-94: exploration noise + clip, one model step, the packed record,
the warm start) checked BY VALUE on every path that computes it, against tests/tail_util.py (float64).

How a case gets its reference: two engines with the same seed (hence the same optimizer draws) are fed the same states at
every control step, one with add_exploration_noise off ("quiet") and one with it on ("noisy").  No optimizer reads the
exploration stream and every warm start comes from the mean, so the quiet engine's action IS the noisy engine's pre-noise
action; prev_mean is asserted equal in both where the optimizer has one.  Then
  noisy action          == tail_util.exploration(quiet action, xi, lo, hi, fix_q7)   within tail_util.action_atol (8 fp32
                           roundings on the magnitudes involved, rtol 0), exactly the bound where the reference clips;
  next_state / reward   == the oracle's model step of the engine's OWN returned action, with the single-step tolerances of
                           test_single_step_random_batch_vs_oracle (pendulum) / test_single_step_matches_oracle (MLP);
for both engines.  xi is injected (tail_util.designed_xi) or the engine's own production draw, which must equal
tail_util.exploration_xi (the documented scheme) bit for bit through dump_noise.  Every case runs complete, ordinary control
steps: 3 of them, noise on at steps 0 and 2 only."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import tail_util as T
from tests.tail_util import ACT, INTENDED_PENDULUM_REWARD, LINEAR_DYNAMICS, MLP_SHAPES
from tests.tail_util import intended_reward as _intended
from tests.tail_util import linear_dynamics_np as _linear_dynamics_np
from tests.tail_util import mlp_bounds as _mlp_bounds
from tests.tail_util import mlp_states as _mlp_states
from tests.tail_util import net as _net
from tests.tail_util import pendulum_states as _pendulum_states

pytestmark = pytest.mark.gpu
F = np.float32
N, H, ITERS, K = 64, 5, 2, 8
SEED = 0x5EED0123456789AB
NOISE_ON = (True, False, True)
P_RTOL = P_ATOL = 1e-5                         # pendulum single step (test_gpu_pendulum.py)
M_RTOL = M_ATOL = 2e-5                         # learned model single step, next state (test_gpu_mlp.py)
MR_RTOL, MR_ATOL = 1e-5, 1e-4                  # ... and its reward


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _opt(L, name):
    """name -> (optimizer, extra quirks, has a warm start the tail writes)"""
    return {"RS": (L.OPT_RANDOM_SEARCH, 0, 0), "CEM": (L.OPT_CEM, 0, 0), "CEM-warm": (L.OPT_CEM, L.FIX_Q2_CEM_WARM_START, 2),
            "PI2": (L.OPT_PI2, 0, 1), "SPSA": (L.OPT_SPSA, 0, 1), "PSO": (L.OPT_PSO, 0, 0), "CMA": (L.OPT_CMAES, 0, 0),
            "CMA-pa": (L.OPT_CMAES, L.CMAES_PER_AGENT, 0)}[name]


def _prev(eng):
    return eng.get_state("prev_mean")


def _close(*engines):
    for e in engines:                            # (a resident kernel would otherwise linger until the handle is collected)
        e.close()


def _run(eng, states, noise_on, xi=None, L=None, between=True, want_prev=False):
    """the control steps of one engine; xi: per-step injected exploration noise (a list), one array for all steps
    (injected once, nothing called between the steps) or None (production draws)"""
    out, prevs, means = [], [], []
    if xi is not None and not isinstance(xi, list):
        eng.inject_noise(L.NOISE_EXPLORATION, xi)
    for t, on in enumerate(noise_on):
        if isinstance(xi, list) and on:
            eng.inject_noise(L.NOISE_EXPLORATION, xi[t])
        out.append(eng.optimize(states[t], t, add_exploration_noise=on))
        if want_prev and between:
            prevs.append(_prev(eng))
            means.append(eng.get_state("mean"))
    if want_prev and not between:
        prevs.append(_prev(eng))
    return out, prevs, means


def _check_records(ev, states, quiet, noisy, noise_on, xis, lo, hi, fix, tols, what, cover=None):
    (s_rt, s_at), (r_rt, r_at) = tols
    for t, on in enumerate(noise_on):
        (qa, qn, qr), (na, nn, nr) = quiet[t], noisy[t]
        w = "%s step %d" % (what, t)
        if on:
            c = T.check_action(na, qa, xis[t], lo, hi, fix, what=w)
            if cover is not None:
                cover += np.array(c)
        else:
            np.testing.assert_array_equal(na, qa, err_msg=w)
        for a, n, r, who in ((qa, qn, qr, "quiet"), (na, nn, nr, "noisy")):
            np.testing.assert_allclose(n, ev.predict_next_state(states[t], a), rtol=s_rt, atol=s_at, err_msg=w + " " + who)
            np.testing.assert_allclose(r, ev.evaluate_next_reward(states[t], n, a), rtol=r_rt, atol=r_at, err_msg=w + " " + who)


def _check_production_draws(L, eng, steps, A, U, agent_offset=0, first=0):
    """the draws of control steps first .. first + steps: dump_noise against the documented scheme, bit for bit"""
    xs = []
    for t in range(first, first + steps):
        x = T.exploration_xi(SEED, t, A, U, agent_offset)
        np.testing.assert_array_equal(eng.dump_noise(L.NOISE_EXPLORATION, t, 0, (A, U)), x, err_msg="control step %d" % t)
        xs.append(x)
    return xs


# ---- analytic pendulum (U = 1): k_finalize_pendulum, k_fused_pendulum (launched and resident), k_fused_pso_pendulum,
# ---- the fused / pending CMA-ES update --------------------------------------------------------------------------
def _pendulum_engine(L, opt_name, A, lo, hi, fix, **kw):
    from blackbox_mpc_amd.engine import Engine
    opt, quirks, _ = _opt(L, opt_name)
    args = dict(dim_s=3, num_agents=A, planning_horizon=H, population_size=N, max_iterations=ITERS, num_elite=K, seed=SEED,
                quirks=quirks | (L.FIX_Q7_EXPL_NOISE_ZERO_MEAN if fix else 0))
    args.update(kw)
    return Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, lo, hi, **args)


# (optimizer, path): path is what the environment asks for and what the engine must then report
PENDULUM_TAILS = [(o, p) for o in ("RS", "CEM", "CEM-warm", "PI2", "SPSA") for p in ("periter", "fused", "resident")] + \
                 [("PSO", "periter"), ("PSO", "fused"), ("CMA", "periter"), ("CMA-pa", "periter"), ("CMA-pa", "fused-cma")]


def _set_path(monkeypatch, path):
    monkeypatch.setenv("BBMPC_FUSED", "0" if path == "periter" else "1")
    monkeypatch.setenv("BBMPC_LINGER_US", "20000" if path == "resident" else "0")      # resident: far longer than the host needs between two calls
    if path == "fused-cma":
        monkeypatch.setenv("BBMPC_CMA_FUSED", "1")


def _assert_path(eng, opt_name, path, A, steps):
    inst = eng.profile_instantiation()
    served, launched = eng.call_stats()
    assert served + launched >= steps
    if path == "resident":
        assert inst.startswith("k_fused_pendulum<") and inst.endswith("true>"), inst
        # one launch, then the mailbox: step 1 (noise off) AND step 2 (noise on) were served by the resident kernel, so both
        # values of the noise flag went through the mailbox (the linger time is far longer than the host takes between calls)
        assert (served, launched) == (steps - 1, 1), (served, launched)
        return
    assert served == 0, (served, launched)
    if path == "fused":
        want = "k_fused_pso_pendulum" if opt_name == "PSO" else "k_fused_pendulum<"
        assert inst.startswith(want) and not inst.endswith("true>"), inst
    elif path == "fused-cma":
        assert inst.startswith("k_fused_cma_pendulum"), inst
    elif opt_name == "CMA-pa" or (opt_name == "CMA" and A == 1):
        # one agent per CMA-ES instance at n <= 32: the rollouts ride on the sampling launch, and exactly then the last update
        # is held back for the tail (launch_pending_cma_update -> k_cma_update_final_small)
        assert inst.startswith("k_cma_sample_roll_small"), inst
    else:
        assert inst.startswith("k_rollout_pendulum"), inst                   # per-iteration kernels + k_finalize_pendulum


def _pendulum_case(L, monkeypatch, opt_name, path, bounds, fix, A, mode, cover=None, reset_first=False):
    lo, hi = T.PENDULUM_BOUNDS[bounds]
    _set_path(monkeypatch, path)
    steps = len(NOISE_ON)
    states = _pendulum_states(steps, A, 11 + A)
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
    warm = _opt(L, opt_name)[2] != 0
    between = path != "resident"                 # any other entry point makes the resident kernel leave: none between its steps
    what = "%s/%s %s fix_q7=%d A=%d %s" % (opt_name, path, bounds, fix, A, mode)
    quiet_eng = _pendulum_engine(L, opt_name, A, lo, hi, fix)
    noisy_eng = _pendulum_engine(L, opt_name, A, lo, hi, fix)
    first = 0
    if reset_first:                              # a reset() restarts the optimizer, not the handle's count of optimize() calls
        for e in (quiet_eng, noisy_eng):         # that keys the draws (rng.hpp): the next control step is number 2
            _run(e, states, (True, True))
            e.reset()
        first = 2
    if mode == "injected":
        xis = [T.designed_xi(A, 1, t) for t in range(steps)]
        xi_arg = xis if between else xis[0]
        if not between:
            xis = [xis[0]] * steps
    else:
        xis = _check_production_draws(L, noisy_eng, steps, A, 1, first=first)
        xi_arg = None
    quiet, q_prev, _ = _run(quiet_eng, states, (False,) * steps, want_prev=warm, between=between)
    noisy, n_prev, _ = _run(noisy_eng, states, NOISE_ON, xi=xi_arg, L=L, want_prev=warm, between=between)
    _assert_path(noisy_eng, opt_name, path, A, steps)
    _assert_path(quiet_eng, opt_name, path, A, steps)
    for i, (a, b) in enumerate(zip(q_prev, n_prev)):
        np.testing.assert_array_equal(a, b, err_msg=what + ": the noise leaked into the warm start (%d)" % i)
    _check_records(ev, states, quiet, noisy, NOISE_ON, xis, lo, hi, fix, ((P_RTOL, P_ATOL), (P_RTOL, P_ATOL)), what, cover)
    _close(quiet_eng, noisy_eng)


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("bounds", list(T.PENDULUM_BOUNDS))
@pytest.mark.parametrize("opt_name,path", PENDULUM_TAILS, ids=["%s-%s" % t for t in PENDULUM_TAILS])
def test_pendulum_tail_by_value(L, monkeypatch, opt_name, path, bounds, fix):
    cover = np.zeros(3, np.int64)
    for mode in ("injected", "production"):
        _pendulum_case(L, monkeypatch, opt_name, path, bounds, fix, 9, mode, cover if mode == "injected" else None)
    # the forcing rows of the designed noise (tests/test_tail_cpu.py) clip on both sides whatever the optimizer returned
    assert cover[0] >= 1 and cover[1] >= 1, cover
    if bounds == "asym":                         # fewer agents: one workgroup / one row, the A = 1 forms of every path
        for A in (1, 3):
            for mode in ("injected", "production"):
                _pendulum_case(L, monkeypatch, opt_name, path, bounds, fix, A, mode)


@pytest.mark.parametrize("opt_name,path", [("CEM", "fused"), ("PI2", "periter"), ("CMA-pa", "periter")])
def test_pendulum_production_draws_after_a_reset(L, monkeypatch, opt_name, path):
    _pendulum_case(L, monkeypatch, opt_name, path, "asym", 0, 3, "production", reset_first=True)


@pytest.mark.parametrize("opt_name,path", [("CEM", "fused"), ("CEM", "periter"), ("PSO", "fused")])
def test_agent_shards_reproduce_the_unsharded_noisy_rows(L, monkeypatch, opt_name, path):
    _set_path(monkeypatch, path)
    lo, hi = T.PENDULUM_BOUNDS["asym"]
    A, steps = 4, len(NOISE_ON)
    states = _pendulum_states(steps, A, 3)
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
    full_q, full_n = _pendulum_engine(L, opt_name, A, lo, hi, 0), _pendulum_engine(L, opt_name, A, lo, hi, 0)
    xis = _check_production_draws(L, full_n, steps, A, 1)
    quiet, _, _ = _run(full_q, states, (False,) * steps)
    noisy, _, _ = _run(full_n, states, NOISE_ON)
    _check_records(ev, states, quiet, noisy, NOISE_ON, xis, lo, hi, 0, ((P_RTOL, P_ATOL), (P_RTOL, P_ATOL)), "unsharded")
    for off in (0, 2):
        sh = _pendulum_engine(L, opt_name, 2, lo, hi, 0, agent_offset=off, num_agents_global=A)
        xs = _check_production_draws(L, sh, steps, 2, 1, agent_offset=off)
        for t in range(steps):
            np.testing.assert_array_equal(xs[t], xis[t][off:off + 2])
        got, _, _ = _run(sh, states[:, off:off + 2], NOISE_ON)
        _close(sh)
        for t in range(steps):
            for g, f in zip(got[t], noisy[t]):
                np.testing.assert_array_equal(g, f[off:off + 2], err_msg="agent_offset %d step %d" % (off, t))
    _close(full_q, full_n)


def test_rollout_episode_matches_the_host_loop_and_the_reference(L, monkeypatch):
    _set_path(monkeypatch, "fused")
    lo, hi = T.PENDULUM_BOUNDS["asym"]
    A, steps = 3, 4
    ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
    for opt_name in ("CEM", "PI2"):
        dev, host, quiet_eng = [_pendulum_engine(L, opt_name, A, lo, hi, 0) for _ in range(3)]
        start = _pendulum_states(1, A, 5)[0]
        acts, nxts, rews = dev.rollout_episode(start, steps, add_exploration_noise=True)
        xis = _check_production_draws(L, dev, steps, A, 1)
        s = start
        for t in range(steps):
            a, n, r = host.optimize(s, t, add_exploration_noise=True)
            for g, w in ((acts[t], a), (nxts[t], n), (rews[t], r)):
                np.testing.assert_array_equal(g, w, err_msg="%s step %d" % (opt_name, t))
            qa, qn, qr = quiet_eng.optimize(s, t)            # the same states, noise off: the pre-noise action
            _check_records(ev, [s], [(qa, qn, qr)], [(a, n, r)], (True,), [xis[t]], lo, hi, 0,
                           ((P_RTOL, P_ATOL), (P_RTOL, P_ATOL)), "%s episode step %d" % (opt_name, t))
            s = n
        _close(dev, host, quiet_eng)


# ---- the user-function route: k_explore + step_dev + k_pack_record + k_shift_left -------------------------------------


def _user_route(L, route):
    """route -> (lo, hi, dynamics kind, oracle evaluator)"""
    if route == "user-reward":
        return T.PENDULUM_BOUNDS["asym"] + (L.DYN_PENDULUM, O.Evaluator(_intended, O.Handler(O.pendulum_dynamics, True)))
    return T.MLP_BOUNDS[2] + (L.DYN_USER, O.Evaluator(_intended, O.Handler(_linear_dynamics_np, True)))


def _user_engine(L, route, opt_name, fix, A):
    from blackbox_mpc_amd.engine import Engine
    opt, quirks, _ = _opt(L, opt_name)
    lo, hi, dyn, _ = _user_route(L, route)
    e = Engine(opt, dyn, L.REW_USER, lo, hi, dim_s=3, num_agents=A, planning_horizon=H, population_size=N,
               max_iterations=ITERS, num_elite=K, seed=SEED, quirks=quirks | (L.FIX_Q7_EXPL_NOISE_ZERO_MEAN if fix else 0))
    if dyn == L.DYN_USER:
        e.set_dynamics_source(LINEAR_DYNAMICS)
    e.set_reward_source(INTENDED_PENDULUM_REWARD)
    return e


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("opt_name", ["RS", "CEM-warm", "PI2"])
@pytest.mark.parametrize("route", ["user-reward", "user-dynamics-U2"])
def test_user_function_route_tail_by_value(L, route, opt_name, fix):
    warm = _opt(L, opt_name)[2]
    A, steps = 9, len(NOISE_ON)
    lo, hi, _, ev = _user_route(L, route)
    U = len(lo)
    states = _pendulum_states(steps, A, 21)
    for mode in ("injected", "production"):
        quiet_eng, noisy_eng = [_user_engine(L, route, opt_name, fix, A) for _ in range(2)]
        if mode == "injected":
            xis = [T.designed_xi(A, U, t) for t in range(steps)]
            xi_arg = xis
        else:
            xis, xi_arg = _check_production_draws(L, noisy_eng, steps, A, U), None
        quiet, q_prev, q_mean = _run(quiet_eng, states, (False,) * steps, want_prev=warm != 0)
        noisy, n_prev, n_mean = _run(noisy_eng, states, NOISE_ON, xi=xi_arg, L=L, want_prev=warm != 0)
        what = "%s %s fix_q7=%d %s" % (route, opt_name, fix, mode)
        assert noisy_eng.call_stats() == (0, steps)
        assert "user" in noisy_eng.profile_instantiation(), noisy_eng.profile_instantiation()
        for t in range(len(q_prev)):
            np.testing.assert_array_equal(n_prev[t], q_prev[t], err_msg=what + ": the noise leaked into the warm start")
            np.testing.assert_array_equal(n_prev[t], T.shift_left(n_mean[t]) if warm == 1 else n_mean[t], err_msg=what)
        cover = np.zeros(3, np.int64)
        _check_records(ev, states, quiet, noisy, NOISE_ON, xis, lo, hi, fix, ((P_RTOL, P_ATOL), (P_RTOL, P_ATOL)), what, cover)
        if mode == "injected":
            assert cover[0] >= 1 and cover[1] >= 1, cover
        _close(quiet_eng, noisy_eng)


# ---- learned dynamics: k_tail_mlp (noisy action + model step + record + warm start in one launch) ------------------------


def _mlp_engine(L, shape, normalized, opt_name, A, fix, **kw):
    from blackbox_mpc_amd.engine import Engine
    dims, acts, S, U, reward = MLP_SHAPES[shape]
    ws, bs, stats, _ = _net(shape, normalized)
    opt, quirks, _ = _opt(L, opt_name)
    lo, hi = _mlp_bounds(U)
    eng = Engine(opt, L.DYN_MLP, L.REW_CHEETAH if reward == "cheetah" else L.REW_PENDULUM, lo, hi, dim_s=S, num_agents=A,
                 planning_horizon=H, population_size=N, max_iterations=ITERS, num_elite=K, seed=SEED,
                 quirks=quirks | (L.FIX_Q7_EXPL_NOISE_ZERO_MEAN if fix else 0), **kw)
    eng.set_mlp(ws, bs, [ACT[a] for a in acts], stats)
    return eng


def _mlp_case(L, shape, normalized, opt_name, fix, A, mode):
    dims, acts, S, U, reward = MLP_SHAPES[shape]
    ev = _net(shape, normalized)[3]
    lo, hi = _mlp_bounds(U)
    warm = _opt(L, opt_name)[2]
    steps = len(NOISE_ON)
    states = _mlp_states(shape, steps, A, 31)
    quiet_eng, noisy_eng = [_mlp_engine(L, shape, normalized, opt_name, A, fix) for _ in range(2)]
    what = "%s norm=%d %s fix_q7=%d A=%d %s" % (shape, normalized, opt_name, fix, A, mode)
    prev0 = _prev(noisy_eng)
    if mode == "injected":
        xis = [T.designed_xi(A, U, t) for t in range(steps)]
        xi_arg = xis
    else:
        xis, xi_arg = _check_production_draws(L, noisy_eng, steps, A, U), None
    quiet, q_prev, q_mean = _run(quiet_eng, states, (False,) * steps, want_prev=True)
    noisy, n_prev, n_mean = _run(noisy_eng, states, NOISE_ON, xi=xi_arg, L=L, want_prev=True)
    assert noisy_eng.call_stats() == (0, steps) and noisy_eng.profile_instantiation().startswith("k_rollout_mlp"), what
    for t in range(steps):
        np.testing.assert_array_equal(n_prev[t], q_prev[t], err_msg=what + ": the noise leaked into the warm start")
        if opt_name != "RS":                     # (RandomSearch keeps no mean)
            np.testing.assert_array_equal(n_mean[t], q_mean[t], err_msg=what)
        if warm == 1:
            np.testing.assert_array_equal(n_prev[t], T.shift_left(n_mean[t]), err_msg=what + " step %d" % t)
        elif warm == 2:
            np.testing.assert_array_equal(n_prev[t], n_mean[t], err_msg=what + " step %d" % t)
        else:
            np.testing.assert_array_equal(n_prev[t], prev0, err_msg=what + ": warm mode 0 leaves prev_mean alone")
    cover = np.zeros(3, np.int64)
    _check_records(ev, states, quiet, noisy, NOISE_ON, xis, lo, hi, fix, ((M_RTOL, M_ATOL), (MR_RTOL, MR_ATOL)), what, cover)
    if mode == "injected":
        assert cover[0] >= 1 and cover[1] >= 1, cover      # the forcing elements clip at hi and at lo whatever the action
    # the record's layout: the action columns hold the action, whatever U (threads 0..U / 64..64+S / 128 of k_tail_mlp)
    assert noisy[0][0].shape == (A, U) and noisy[0][1].shape == (A, S) and noisy[0][2].shape == (A,)
    _close(quiet_eng, noisy_eng)


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("opt_name", ["RS", "CEM", "PI2", "SPSA", "CEM-warm"])
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("shape", ["S20-U6-h200", "S3-U2-h16"])
def test_learned_model_tail_by_value(L, shape, normalized, opt_name, fix):
    for mode in ("injected", "production"):
        _mlp_case(L, shape, normalized, opt_name, fix, 3, mode)


@pytest.mark.parametrize("opt_name", ["PI2", "SPSA", "CEM-warm"])
@pytest.mark.parametrize("route", ["learned", "user-reward", "user-dynamics-U2"])
def test_traced_mean_is_what_the_warm_start_shifts(L, route, opt_name):
    # The by-value cases above compare prev_mean with get_state("mean"), not with the parity trace: set_trace() takes a handle
    # off the very paths they are about (the skipped k_dist_init of PI2, the graph-replayed step, the host-polled record).
    # Here the trace is on, warm modes 1 and 2 on both routes that fuse the warm start into the tail: the last traced mean is
    # the tensor get_state("mean") returns, and prev_mean is its shift / copy, with noise on and off.
    shape, A = "S3-U2-h16", 3
    warm = _opt(L, opt_name)[2]
    eng = _mlp_engine(L, shape, True, opt_name, A, 0) if route == "learned" else _user_engine(L, route, opt_name, 0, A)
    eng.set_trace(True)
    states = _mlp_states(shape, len(NOISE_ON), A, 33)
    for t, on in enumerate(NOISE_ON):
        eng.optimize(states[t], t, add_exploration_noise=on)
        traced = eng.get_trace(ITERS - 1, L.TRACE_MEAN)
        np.testing.assert_array_equal(eng.get_state("mean"), traced, err_msg="step %d" % t)
        np.testing.assert_array_equal(_prev(eng), T.shift_left(traced) if warm == 1 else traced, err_msg="step %d" % t)
    _close(eng)


@pytest.mark.parametrize("opt_name", ["PI2", "CEM"])
def test_graph_replayed_step_by_value(L, monkeypatch, opt_name):
    # learned-model PI2 / CEM through bbmpc_optimize: after three identical calls the control step is captured and replayed
    # as a graph whose Philox control-step word lives in device memory (RngKey::step_src, advanced by k_tail_mlp's last
    # workgroup).  Every replay must use ITS step's draw: the device's count stays in line with the host's.
    monkeypatch.setenv("BBMPC_STEP_GRAPH", "1")
    shape, A, steps = "S20-U6-h200", 3, 9
    dims, acts, S, U, reward = MLP_SHAPES[shape]
    ev = _net(shape, True)[3]
    lo, hi = _mlp_bounds(U)
    states = _mlp_states(shape, steps, A, 35)
    quiet_eng, noisy_eng = [_mlp_engine(L, shape, True, opt_name, A, 0) for _ in range(2)]
    xis = _check_production_draws(L, noisy_eng, steps, A, U)
    on = (True,) * steps
    quiet, _, _ = _run(quiet_eng, states, (False,) * steps)
    noisy, _, _ = _run(noisy_eng, states, on)
    assert noisy_eng.graph_stats() >= 4, noisy_eng.graph_stats()
    _check_records(ev, states, quiet, noisy, on, xis, lo, hi, 0, ((M_RTOL, M_ATOL), (MR_RTOL, MR_ATOL)), "graph " + opt_name)
    # one more call outside the graph (noise off: another signature, launched kernel by kernel) and one back inside (the
    # captured graph again, after the host has put the device's step word back in line): host and device still agree
    xs = [T.exploration_xi(SEED, steps + i, A, U) for i in range(2)]
    for i, flag in enumerate((False, True)):
        s = states[i]
        before = noisy_eng.graph_stats()
        q = quiet_eng.optimize(s, steps + i)
        n = noisy_eng.optimize(s, steps + i, add_exploration_noise=flag)
        assert noisy_eng.graph_stats() == before + (1 if flag else 0), (flag, before, noisy_eng.graph_stats())
        _check_records(ev, [s], [q], [n], (flag,), [xs[i]], lo, hi, 0, ((M_RTOL, M_ATOL), (MR_RTOL, MR_ATOL)), "graph %s after %d" % (opt_name, i))
    _close(quiet_eng, noisy_eng)


@pytest.mark.parametrize("opt_name", ["RS", "PI2"])
@pytest.mark.parametrize("shape", ["S64-U64-h96", "S3-U125-h96"])
def test_widest_learned_model_tail_by_value(L, shape, opt_name):
    for mode in ("injected", "production"):
        _mlp_case(L, shape, True, opt_name, 0, 2, mode)
