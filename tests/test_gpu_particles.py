"""Particle trajectory evaluator on the GPU (include/bbmpc.h: bbmpc_set_particles): the process-noise generator against
its documented definition, per-particle returns and scores against the NumPy statement of tests/particle_util.py with
injected noise, the optimizers in lock-step with the oracle's, sharding, refusals and the Python classes."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import particle_util as PU
from tests.parity_util import assert_cheetah_rewards
from tests.test_particles_cpu import AGG_SIGMA, PEND_SHAPES, PEND_SIGMA, R_ATOL, R_RTOL, pendulum_case

pytestmark = pytest.mark.gpu

F = np.float32
LO, HI = [-2.0], [2.0]
STRICT_MATH = 1 << 9


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device visible"
    return _lib


def _engine(L, opt, A, H, N=0, iters=0, k=0, **kw):
    from blackbox_mpc_amd.engine import Engine
    return Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, LO, HI, dim_s=3, num_agents=A, planning_horizon=H,
                  population_size=N, max_iterations=iters, num_elite=k, **kw)


def _pendulum_ev():
    return O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))


def _helper(eps, P, sigma, kappa, ev=None):
    ev = ev or _pendulum_ev()
    return PU.ParticleEvaluator(ev.reward, ev.handler, P, sigma, kappa, eps)


# ---- 1. generator ---------------------------------------------------------------------------------------------------
def test_process_noise_matches_the_documented_scheme(L):
    A, P, H, S = 2, 3, 5, 3                                   # H * S = 15: a ragged last Philox block
    seed = 0x1234567890ABCDEF
    eng = _engine(L, L.OPT_CEM, A, H, N=8, iters=2, k=2, seed=seed, agent_offset=5)
    eng.set_particles(P, PEND_SIGMA)
    for step, it in [(0, 0), (3, 1)]:
        got = eng.dump_noise(L.NOISE_PROCESS, step, it, (A, P, H, S))
        want = PU.process_noise_np(seed, step, it, A, P, H, S, agent_offset=5)
        # float32 Box-Muller: the angle 2 pi u is rounded to 4.8e-7, times a radius of at most sqrt(2 ln 2^24) = 5.8, and
        # log / sqrt / sincos add a few ulp of that radius
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    with pytest.raises(L.BBMPCError):
        eng.dump_noise(L.NOISE_PROCESS, 0, 0, (A, P, H))
    # equal calls, equal bits: bbmpc_evaluate draws with iteration 0 and the handle's current control step
    states, seq, _ = pendulum_case(9, A, P, H)
    np.testing.assert_array_equal(eng.evaluate(states, seq), eng.evaluate(states, seq))


# ---- 2. per-particle returns, injected eps --------------------------------------------------------------------------
@pytest.mark.parametrize("N,A,P,H", PEND_SHAPES)
def test_pendulum_particle_returns_match_the_helper(L, N, A, P, H):
    states, seq, eps = pendulum_case(N, A, P, H)
    eng = _engine(L, L.OPT_NONE, A, H)
    eng.set_particles(P, PEND_SIGMA, 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    scores, got = eng.evaluate_particles(states, seq)
    assert got.shape == (N, P, A) and scores.shape == (N, A)
    want = PU.particle_returns(_pendulum_ev(), states, seq, eps, PEND_SIGMA, P)
    # the rule of parity_util.assert_pendulum_rewards: what misses the tolerance must be rare and at least as close to the
    # float64 recurrence as the float32 helper is
    g, w = got.astype(np.float64), want.astype(np.float64)
    tol = R_ATOL + R_RTOL * np.abs(w)
    bad = np.abs(g - w) > tol
    print("[particles pendulum N=%d A=%d P=%d H=%d] max |dev - helper| = %.3e, outside the tolerance: %d of %d"
          % (N, A, P, H, np.abs(g - w).max(), int(bad.sum()), bad.size))
    if bad.any():
        assert bad.mean() <= 0.01
        exact = PU.pendulum_particle_returns64(states, seq, eps, PEND_SIGMA.astype(np.float64), P)
        assert not (bad & (np.abs(g - exact) > np.abs(w - exact) + tol)).any()
    np.testing.assert_array_equal(eng.evaluate(states, seq), scores)          # bbmpc_evaluate returns the scores


def _mlp_problem(L, spec, A, H, **kw):
    from tests.test_gpu_mlp import _problem
    dims, acts, S, U, reward = spec
    eng, ev, lo, hi = _problem(L, dims, acts, S, U, reward, True, A=A, H=H, **kw)
    return eng, ev, S, U, reward


def _mlp_specs():
    from tests.test_ensemble_cpu import NARROW_NET
    from tests.test_gpu_mlp import CHEETAH, PEND_MLP
    # cheetah: 15 and 148 rows per agent in 16-row tiles that mix candidates, the second with a partial last tile; the narrow
    # net: one wave, noise and actions on the fall-back fetches (tests/test_ensemble_cpu.py, also for how its inputs were checked)
    return [(CHEETAH, 5, 1, 3, 2), (CHEETAH, 37, 3, 4, 12), (PEND_MLP, 33, 2, 16, 9), (NARROW_NET, 5, 2, 4, 3)]


@pytest.mark.parametrize("case", range(4))
def test_mlp_particle_returns_match_the_helper(L, case):
    spec, N, A, P, H = _mlp_specs()[case]
    eng, ev, S, U, reward = _mlp_problem(L, spec, A, H)
    rng = np.random.default_rng(1000 + case)
    states = (O.cheetah_start_states(A, S) if reward == "cheetah" else O.pendulum_start_states(A)).astype(F)
    seq = rng.uniform(-1, 1, (N, A, H, U)).astype(F)
    eps = rng.standard_normal((A, P, H, S)).astype(F)
    sigma = np.full(S, 0.02, F)
    eng.set_particles(P, sigma, 0.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    _, got = eng.evaluate_particles(states, seq)
    want, visited = PU.particle_returns(ev, states, seq, eps, sigma, P, keep_states=True)
    print("[particles mlp case %d] max |dev - helper| = %.3e" % (case, np.abs(got.astype(np.float64) - want).max()))
    if reward == "cheetah":
        assert_cheetah_rewards(got.reshape(N * P, A), want.reshape(N * P, A), 1e-3, 1e-3 * H,
                               margin=lambda: PU.cheetah_noisy_margin(visited).reshape(N * P, A))
    else:
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * H)


# ---- 3. aggregate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", [0.0, 1.5])
def test_scores_are_the_aggregate_of_the_returns(L, kappa):
    N, A, P, H = 257, 2, 8, 20
    states, seq, eps = pendulum_case(N, A, P, H)
    eng = _engine(L, L.OPT_NONE, A, H)
    eng.set_particles(P, AGG_SIGMA, kappa)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    scores, returns = eng.evaluate_particles(states, seq)
    bound, rows = PU.aggregate_bound(returns, kappa)
    assert rows.mean() >= 0.9
    err = np.abs(scores.astype(np.float64) - PU.aggregate64(returns, kappa))
    print("[particles aggregate kappa=%g] max err / bound = %.3e on %d of %d rows" % (kappa, (err[rows] / bound[rows]).max(), rows.sum(), rows.size))
    assert np.all(err[rows] <= bound[rows])
    # one NaN particle (its noise path is NaN from step 3 on): -1e6 for that particle of every candidate of agent 1, the
    # others untouched, and a finite score that follows the formula
    eps_nan = eps.copy()
    eps_nan[1, 5, 3, 2] = np.nan
    eng.inject_noise(L.NOISE_PROCESS, eps_nan)
    s2, r2 = eng.evaluate_particles(states, seq)
    assert np.all(r2[:, 5, 1] == F(-1e6))
    keep = np.ones(P, bool)
    keep[5] = False
    np.testing.assert_array_equal(r2[:, keep, :], returns[:, keep, :])
    np.testing.assert_array_equal(r2[:, :, 0], returns[:, :, 0])
    assert np.all(np.isfinite(s2))
    np.testing.assert_allclose(s2, PU.aggregate64(r2, kappa), rtol=1e-5)


def test_nan_weight_gives_minus_1e6_per_particle(L):
    from tests.test_gpu_mlp import PEND_MLP, ACT
    dims, acts, S, U, _ = PEND_MLP
    eng, ev, S, U, _ = _mlp_problem(L, PEND_MLP, 1, 4)
    ws, bs = O.make_mlp_params(dims, seed=42)
    ws[1][3, 5] = np.nan
    eng.set_mlp(ws, bs, [ACT[a] for a in acts], None)
    eng.set_particles(3, np.full(S, 0.02, F), 1.5)
    scores, returns = eng.evaluate_particles(O.pendulum_start_states(1), np.zeros((5, 1, 4, 1), F))
    assert np.all(returns == F(-1e6)) and np.all(scores == F(-1e6))      # mean -1e6, variance 0


# ---- 4. degenerate cases --------------------------------------------------------------------------------------------
def test_zero_sigma_is_the_deterministic_evaluator(L, monkeypatch):
    monkeypatch.setenv("BBMPC_FUSED", "0")
    N, A, H = 65, 3, 7
    states, seq, _ = pendulum_case(N, A, 2, H)
    det = _engine(L, L.OPT_NONE, A, H, quirks=STRICT_MATH)
    eng = _engine(L, L.OPT_NONE, A, H)
    eng.set_particles(2, np.zeros(3, F), 0.0)
    np.testing.assert_allclose(eng.evaluate(states, seq), det.evaluate(states, seq), rtol=R_RTOL, atol=R_ATOL)
    from tests.test_gpu_mlp import CHEETAH
    meng, ev, S, U, _ = _mlp_problem(L, CHEETAH, 2, 6)
    rng = np.random.default_rng(4)
    mstates, mseq = O.cheetah_start_states(2, S).astype(F), rng.uniform(-1, 1, (37, 2, 6, U)).astype(F)
    want = meng.evaluate(mstates, mseq)
    meng.set_particles(2, np.zeros(S, F), 0.0)
    from tests.parity_util import cheetah_threshold_margin
    assert_cheetah_rewards(meng.evaluate(mstates, mseq), want, 1e-3, 1e-3 * 6, margin=lambda: cheetah_threshold_margin(ev, mstates, mseq))
    # num_particles = 0 after use: the deterministic results, bit for bit
    meng.set_particles(0)
    np.testing.assert_array_equal(meng.evaluate(mstates, mseq), want)
    base = _engine(L, L.OPT_NONE, A, H).evaluate(states, seq)
    eng.set_particles(0)
    np.testing.assert_array_equal(eng.evaluate(states, seq), base)


def test_switching_particles_off_restores_the_control_step(L):
    N, A, H, iters, k = 128, 2, 8, 3, 16
    eng = _engine(L, L.OPT_CEM, A, H, N=N, iters=iters, k=k)
    rng = np.random.default_rng(2)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack([O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]))
    s = O.pendulum_start_states(A)
    first = eng.optimize(s)                 # CEM restarts from its constructor distribution (quirk Q2): same draws, same step
    eng.set_particles(4, AGG_SIGMA, 1.0)
    noisy = eng.optimize(s)
    assert np.all(np.isfinite(noisy[0])) and not np.array_equal(noisy[0], first[0])
    eng.set_particles(0)
    again = eng.optimize(s)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)


# ---- 5. optimizers, injected draws ----------------------------------------------------------------------------------
def test_random_search_lockstep(L):
    N, A, H, P = 64, 2, 6, 4
    rng = np.random.default_rng(5)
    eps = rng.standard_normal((1, A, P, H, 3)).astype(F)
    u01 = rng.random((N, A, H, 1)).astype(F)
    eng = _engine(L, L.OPT_RANDOM_SEARCH, A, H, N=N)
    eng.set_trace(True)
    eng.set_particles(P, AGG_SIGMA, 1.0)
    eng.inject_noise(L.NOISE_UNIFORM, u01)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    rs = O.RandomSearch(_helper(eps, P, AGG_SIGMA, 1.0), LO, HI, horizon=H, population=N, num_agents=A)
    act_o, nxt_o, rew_o = rs.call(states, {"uniform": u01})
    np.testing.assert_array_equal(eng.get_trace(0, L.TRACE_SAMPLES), rs.trace[0]["samples"])
    np.testing.assert_allclose(eng.get_trace(0, L.TRACE_REWARDS), rs.trace[0]["rewards"], rtol=R_RTOL, atol=R_ATOL)
    np.testing.assert_array_equal(eng.get_trace(0, L.TRACE_ELITES), rs.trace[0]["best"])
    np.testing.assert_array_equal(act, act_o)
    # the record stays the noise-free one-step prediction
    np.testing.assert_allclose(nxt, nxt_o, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(rew, rew_o, rtol=1e-5, atol=1e-5)


def test_pi2_lockstep(L):
    N, A, H, iters, P = 128, 2, 8, 3, 4
    rng = np.random.default_rng(23)
    eps = rng.standard_normal((iters, A, P, H, 3)).astype(F)
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]}
    eng = _engine(L, L.OPT_PI2, A, H, N=N, iters=iters)
    eng.set_trace(True)
    eng.set_particles(P, AGG_SIGMA, 0.5)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    eng.inject_noise(L.NOISE_PROCESS, eps)
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    hip_r = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(iters)]

    def lock(it, r_o):
        np.testing.assert_allclose(hip_r[it], r_o, rtol=R_RTOL, atol=R_ATOL)
        return hip_r[it]
    pi2 = O.PI2(_helper(eps, P, AGG_SIGMA, 0.5), LO, HI, horizon=H, max_iterations=iters, population=N, num_agents=A)
    act_o = pi2._optimize(states, noise, rewards_override=lock)
    for it in range(iters):
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_SAMPLES), pi2.trace[it]["samples"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), pi2.trace[it]["mean"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(act, act_o, rtol=0, atol=2e-5)
    np.testing.assert_allclose(eng.get_state("prev_mean"), pi2.prev, rtol=0, atol=2e-5)


def test_cem_lockstep(L):
    N, A, H, iters, k, P = 128, 1, 8, 3, 16, 4
    rng = np.random.default_rng(17)
    eps = rng.standard_normal((iters, A, P, H, 3)).astype(F)
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]}
    eng = _engine(L, L.OPT_CEM, A, H, N=N, iters=iters, k=k)
    eng.set_trace(True)
    eng.set_particles(P, AGG_SIGMA, 0.5)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    eng.inject_noise(L.NOISE_PROCESS, eps)
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    hip_el = [eng.get_trace(it, L.TRACE_ELITES) for it in range(iters)]
    hip_r = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(iters)]

    def select(it, r_o, own):                            # the forced-elites hook of tests/test_gpu_pendulum.py
        np.testing.assert_allclose(hip_r[it], r_o, rtol=R_RTOL, atol=R_ATOL)
        for a in range(A):
            he = hip_el[it][a]
            if set(own[a]) != set(he):
                kth = np.sort(r_o[:, a])[::-1][k - 1]
                for n in set(own[a]) ^ set(he):
                    assert abs(r_o[n, a] - kth) <= R_ATOL + R_RTOL * abs(kth)
            np.testing.assert_array_equal(he, O.topk_desc(hip_r[it][:, a], k))
        return hip_el[it]
    cem = O.CEM(_helper(eps, P, AGG_SIGMA, 0.5), LO, HI, horizon=H, max_iterations=iters, population=N, num_elite=k, num_agents=A)
    cem._optimize(states, noise, forced_elites=select)
    for it in range(iters):
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_SAMPLES), cem.trace[it]["samples"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), cem.trace[it]["mean"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(eng.get_trace(it, L.TRACE_VAR), cem.trace[it]["var"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(act, cem.trace[-1]["mean"][:, 0], rtol=0, atol=2e-5)


@pytest.mark.parametrize("opt_name", ["PSO", "SPSA", "CMAES"])
def test_other_optimizers_score_through_the_particles(L, opt_name):
    """One control step at sigma > 0: it completes, the traced rewards of iteration 0 are what evaluate_particles gives for
    the candidates that iteration rolled out (minus their bound penalty), the action is finite and inside the bounds."""
    N, A, H, P = 32, 1, 6, 4
    rng = np.random.default_rng(31)
    eps = rng.standard_normal((1, A, P, H, 3)).astype(F)
    opt = {"PSO": L.OPT_PSO, "SPSA": L.OPT_SPSA, "CMAES": L.OPT_CMAES}[opt_name]
    eng = _engine(L, opt, A, H, N=N, iters=1, k=8)
    eng.set_trace(True)
    eng.set_particles(P, AGG_SIGMA, 1.0)
    eng.inject_noise(L.NOISE_PROCESS, eps)
    pen = np.zeros((N, A), F)
    if opt_name == "PSO":                                 # the constructor's swarm: every position zero (quirk Q4)
        cands = [np.zeros((N, A, H, 1), F)]
    elif opt_name == "SPSA":                              # mean (the bounds' midpoint, 0) +- c_0 * delta, c_0 = spsa_c = 0.3
        delta = np.where(rng.random((N, A, H, 1)) < 0.5, F(-1), F(1)).astype(F)
        eng.inject_noise(L.NOISE_RADEMACHER, delta[None])
        cands = [(F(0.3) * delta).astype(F), (F(-0.3) * delta).astype(F)]
    else:                                                 # m + sigma * B D z with m = 0, sigma = 1, B = D = I: the draws
        z = rng.standard_normal((N, A, H, 1)).astype(F)
        eng.inject_noise(L.NOISE_NORMAL, z[None])
        feas = np.clip(z, F(-2), F(2))
        d = (z - feas).reshape(N, A, -1)
        nrm = O.sqrt32(O.seq_sum((d * d).astype(F), axis=2))
        pen = (nrm * nrm).astype(F)
        assert pen.max() > 0
        cands = [feas]
    states = O.pendulum_start_states(A)
    act, nxt, rew = eng.optimize(states)
    traced = eng.get_trace(0, L.TRACE_REWARDS)
    assert np.all(np.isfinite(act)) and np.all(act >= -2.0) and np.all(act <= 2.0) and np.all(np.isfinite(nxt))
    want = np.concatenate([(eng.evaluate_particles(states, c)[0] - pen).astype(F) for c in cands])
    np.testing.assert_allclose(traced, want, rtol=1e-6, atol=1e-5)


# ---- 6. sharding ----------------------------------------------------------------------------------------------------
def test_agent_sharding_is_bit_identical(L):
    N, A, P, H = 40, 2, 5, 7
    states, seq, _ = pendulum_case(N, A, P, H)
    whole = _engine(L, L.OPT_NONE, A, H, seed=99)
    whole.set_particles(P, AGG_SIGMA, 1.5)
    want = whole.evaluate(states, seq)
    for a in range(A):
        shard = _engine(L, L.OPT_NONE, 1, H, seed=99, agent_offset=a, num_agents_global=A)
        shard.set_particles(P, AGG_SIGMA, 1.5)
        np.testing.assert_array_equal(shard.evaluate(states[a:a + 1], seq[:, a:a + 1])[:, 0], want[:, a])
    assert np.any(want[:, 0] != want[:, 1])


# ---- 7. risk --------------------------------------------------------------------------------------------------------
def test_risk_term_is_what_the_optimizer_sees(L):
    """Two candidates under the same eight noise paths: A has the higher mean return and the higher spread, B the reverse
    (margins of 1.8 in both orderings, against a rollout tolerance of 2e-2).  RandomSearch takes A at kappa = 0 and B at
    kappa = 3."""
    H, P = 10, 8
    sigma = np.array([0.05, 0.05, 0.5], F)
    rng = np.random.default_rng(77)
    eps = rng.standard_normal((1, P, H, 3)).astype(F)
    u01 = rng.random((400, 1, H, 1)).astype(F)[[273, 259]]
    states = O.pendulum_start_states(1)
    seq = ((u01 * F(4.0)).astype(F) + F(-2.0)).astype(F)
    r = PU.particle_returns(_pendulum_ev(), states, seq, eps, sigma, P)[:, :, 0].astype(np.float64)
    m, s = r.mean(axis=1), r.std(axis=1)
    assert m[0] - m[1] > 1.0 and s[0] > s[1] and (m[1] - 3 * s[1]) - (m[0] - 3 * s[0]) > 1.0
    picks = {}
    for kappa in (0.0, 3.0):
        eng = _engine(L, L.OPT_RANDOM_SEARCH, 1, H, N=2)
        eng.set_trace(True)
        eng.set_particles(P, sigma, kappa)
        eng.inject_noise(L.NOISE_UNIFORM, u01)
        eng.inject_noise(L.NOISE_PROCESS, eps[None])
        act, _, _ = eng.optimize(states)
        picks[kappa] = int(eng.get_trace(0, L.TRACE_ELITES)[0])
        np.testing.assert_array_equal(act[0], seq[picks[kappa], 0, 0])
    assert picks == {0.0: 0, 3.0: 1}


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(L):
    from blackbox_mpc_amd.engine import Engine
    sigma = np.full(3, 0.1, F)
    states, seq, _ = pendulum_case(4, 1, 2, 5)
    reward_src = """
__device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) { return -nxt[2] * nxt[2]; }
"""
    user = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_USER, LO, HI, dim_s=3, num_agents=1, planning_horizon=5)
    user.set_reward_source(reward_src)
    before = user.evaluate(states, seq)
    with pytest.raises(L.BBMPCError) as ei:
        user.set_particles(2, sigma)
    assert ei.value.code == L.E_UNSUPPORTED and "reward" in str(ei.value)
    np.testing.assert_array_equal(user.evaluate(states, seq), before)

    from tests.test_gpu_mlp import PEND_MLP
    mlp, ev, S, U, _ = _mlp_problem(L, PEND_MLP, 1, 5)
    mlp.set_inverse_transform_source("""
__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {
    for (int i = 0; i < S; ++i) next[i] = cur[i] + dev[i];
}
""")
    before = mlp.evaluate(states, seq)
    with pytest.raises(L.BBMPCError) as ei:
        mlp.set_particles(2, sigma)
    assert ei.value.code == L.E_UNSUPPORTED and "transform" in str(ei.value)
    np.testing.assert_array_equal(mlp.evaluate(states, seq), before)

    shard = _engine(L, L.OPT_PI2, 1, 5, N=16, iters=1, population_offset=0, population_global=32)
    with pytest.raises(L.BBMPCError) as ei:
        shard.set_particles(2, sigma)
    assert ei.value.code == L.E_UNSUPPORTED and "sharded" in str(ei.value)

    eng = _engine(L, L.OPT_RANDOM_SEARCH, 1, 5, N=1024)
    with pytest.raises(L.BBMPCError) as ei:
        eng.set_particles(64, sigma)                      # 65536 rows per agent
    assert ei.value.code == L.E_UNSUPPORTED
    for bad in ((65, sigma, 0.0), (-1, sigma, 0.0), (2, -sigma, 0.0), (2, np.array([0.1, np.inf, 0.1], F), 0.0), (2, sigma, np.nan)):
        with pytest.raises(L.BBMPCError) as ei:
            eng.set_particles(*bad)
        assert ei.value.code == L.E_INVALID
    with pytest.raises(L.BBMPCError) as ei:               # the layout depends on num_particles: set them first
        eng.inject_noise(L.NOISE_PROCESS, np.zeros((1, 2, 5, 3), F))
    assert ei.value.code == L.E_STATE
    act, _, _ = eng.optimize(states)
    assert np.all(np.isfinite(act))
    eng.set_particles(2, sigma)
    with pytest.raises(L.BBMPCError) as ei:
        eng.inject_noise(L.NOISE_PROCESS, np.zeros((1, 3, 5, 3), F))
    assert ei.value.code == L.E_INVALID
    act, _, _ = eng.optimize(states)
    assert np.all(np.isfinite(act))


# ---- 9. Python ------------------------------------------------------------------------------------------------------
def test_mpc_policy_with_the_particle_evaluator(L):
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.trajectory_evaluators import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    act_space, obs_space = Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8])
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=PendulumTrueModel(), true_model=True)
    sigma = [0.02, 0.02, 0.2]
    ev = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=4, process_noise_std=sigma, risk_kappa=1.0)
    pol = MPCPolicy(trajectory_evaluator=ev, env_action_space=act_space, env_observation_space=obs_space,
                    optimizer_name="CEM", num_agents=1, planning_horizon=8, population_size=64, max_iterations=2,
                    num_elite=8, seed=11)
    eng = _engine(L, L.OPT_CEM, 1, 8, N=64, iters=2, k=8, seed=11)
    eng.set_particles(4, np.array(sigma, F), 1.0)
    obs = np.array([1.0, 0.0, 0.0], F)
    oracle = _pendulum_ev()
    for t in range(10):
        a, n, r = pol.act(obs, t)
        a_e, n_e, r_e = eng.optimize(obs[None])
        np.testing.assert_array_equal(a, a_e[0])
        np.testing.assert_array_equal(n, n_e[0])
        np.testing.assert_array_equal(r, r_e[0])
        obs = oracle.predict_next_state(obs[None], a[None].astype(F))[0]
    # the evaluator's own calls: scores, per-particle returns, and the deterministic one-step API
    seq = np.random.default_rng(3).uniform(-2, 2, (9, 1, 8, 1)).astype(F)
    scores = ev(obs[None], seq)
    returns = ev.particle_returns(obs[None], seq)
    assert scores.shape == (9, 1) and returns.shape == (9, 4, 1)
    np.testing.assert_allclose(scores, PU.aggregate64(returns, 1.0), rtol=1e-5)
    np.testing.assert_allclose(ev.predict_next_state(obs[None], seq[:1, 0, 0]), oracle.predict_next_state(obs[None], seq[:1, 0, 0]),
                               rtol=1e-5, atol=1e-5)
