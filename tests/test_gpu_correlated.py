"""GPU tests of temporally correlated sampling for CEM / PI2 (bbmpc_set_sampling_correlation), through
the C ABI, against the NumPy statements of tests/correlated_util.py.

Shapes: N = 70 (two 64-candidate workgroups of k_gen_candidates_corr, the second partial), A = 2, H = 5, 2 iterations; the
analytic pendulum (U = 1) and a tiny learned model with U = 5 (so that j = s * U + u indexing is exercised).

Bounds: traced samples against the float64 statement within
    2^-23 * ((H + 2) * sigma * sum_s |M[t,s] z[s]| + |want|)
(correlated_util.sample_bound: the sequential-sum error bound with a factor 2 of slack); everything behind the samples with
the tolerances the uncorrelated paths are held to (tests/test_gpu_pendulum.py, tests/test_gpu_mlp.py,
tests/test_particles_cpu.py, tests/test_gpu_user_functions.py)."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import correlated_util as CU
from tests.parity_util import assert_cheetah_rewards, cheetah_threshold_margin
from tests.test_particles_cpu import R_ATOL, R_RTOL                   # pendulum H-step rewards: rtol 2e-4, atol 2e-3

pytestmark = pytest.mark.gpu
F = np.float32
N, A, H, ITERS, K = 70, 2, 5, 2, 8
TINY_MLP = ([23, 40, 18], ["tanh", None], 18, 5, "cheetah")           # S = 18, U = 5: one of tests/test_gpu_mlp.py's shapes
MLP_R_RTOL, MLP_R_ATOL = 1e-3, 1e-3 * H                              # tests/test_gpu_mlp.py: H-step rewards of the learned model


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _mix(seed=0):
    """dense, asymmetric (a transposed read fails), row sums of |M| above 1 (CEM draws leave the bounds and are clipped)"""
    return np.random.default_rng(100 + seed).normal(0.0, 0.8, (H, H)).astype(F)


class Problem:
    def __init__(self, L, model, opt_name, reward_source=None, **kw):
        from blackbox_mpc_amd.engine import Engine
        self.opt_name = opt_name
        opt = {"CEM": L.OPT_CEM, "PI2": L.OPT_PI2}[opt_name]
        k = K if opt_name == "CEM" else 0
        if model == "pendulum":
            self.lo, self.hi, self.S, self.U = [-2.0], [2.0], 3, 1
            rk = L.REW_USER if reward_source else L.REW_PENDULUM
            self.eng = Engine(opt, L.DYN_PENDULUM, rk, self.lo, self.hi, dim_s=3, num_agents=A, planning_horizon=H,
                              population_size=N, max_iterations=ITERS, num_elite=k, **kw)
            if reward_source:
                self.eng.set_reward_source(reward_source)
            self.ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
            self.states = O.pendulum_start_states(A)
        else:
            from tests.test_gpu_mlp import _problem
            dims, acts, S, U, reward = TINY_MLP
            self.eng, self.ev, self.lo, self.hi = _problem(L, dims, acts, S, U, reward, True, A=A, H=H, opt=opt, N=N, iters=ITERS,
                                                           k=k, **kw)
            self.S, self.U = S, U
            self.states = O.cheetah_start_states(A, S).astype(F)
        self.model = model
        self.lo_h = np.tile(np.asarray(self.lo, F)[None], (H, 1))
        self.hi_h = np.tile(np.asarray(self.hi, F)[None], (H, 1))

    def oracle(self, mix=None, **kw):
        if self.opt_name == "CEM":
            if mix is None:
                return O.CEM(self.ev, self.lo, self.hi, horizon=H, max_iterations=ITERS, population=N, num_elite=K, num_agents=A, **kw)
            return CU.CorrelatedCEM(self.ev, self.lo, self.hi, horizon=H, max_iterations=ITERS, population=N, num_elite=K,
                                    num_agents=A, mix=mix, **kw)
        return O.PI2(self.ev, self.lo, self.hi, horizon=H, max_iterations=ITERS, population=N, num_agents=A, **kw)

    def noise(self, seed):
        rng = np.random.default_rng(seed)
        return {"trunc": [O.truncated_normal_noise(rng, (N, A, H, self.U)) for _ in range(ITERS)]}


def _check_samples(L, p, M, z_per_iter, what):
    """traced samples of every iteration of control step 0 against the float64 statement, from the traced mean / var of
    the iteration before (the constructor distribution for iteration 0); returns how many elements were clipped"""
    eng, base = p.eng, p.oracle()
    mean, var = base._init_mean(), base._init_var()
    clipped = 0
    for it in range(ITERS):
        sigma = CU.cem_sigma32(mean, var, p.lo_h, p.hi_h) if p.opt_name == "CEM" else O.sqrt32(var)
        want, mag, raw = CU.candidates64(M, z_per_iter[it], sigma, mean, p.lo_h, p.hi_h)    # CEM clips; PI2 stores the feasible samples
        got = eng.get_trace(it, L.TRACE_SAMPLES).astype(np.float64)
        err, bound = np.abs(got - want), CU.sample_bound(H, mag, want)
        print("[%s it %d] max |got - want| / bound = %.3f, clipped %d of %d" % (what, it, (err / bound).max(), int((raw != want).sum()), raw.size))
        assert np.all(err <= bound), "%s iteration %d: %d samples outside the bound (worst %.3e vs %.3e)" % (
            what, it, int((err > bound).sum()), err.max(), bound[np.unravel_index(err.argmax(), err.shape)])
        out = raw != want
        assert np.array_equal(got[out], want[out])                                 # a clipped element IS the bound
        clipped += int(out.sum())
        mean = eng.get_trace(it, L.TRACE_MEAN)
        if p.opt_name == "CEM":
            var = eng.get_trace(it, L.TRACE_VAR)
    return clipped


CASES = [("pendulum", "CEM"), ("pendulum", "PI2"), ("mlp", "CEM"), ("mlp", "PI2")]


# ---- 1. samples, injected noise, dense asymmetric M ------------------------------------------------------------------
@pytest.mark.parametrize("model,opt_name", CASES)
def test_samples_follow_the_rule_with_injected_noise(L, model, opt_name):
    p = Problem(L, model, opt_name)
    M = _mix()
    noise = p.noise(1)
    p.eng.set_trace(True)
    p.eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    assert not p.eng.sampling_correlation_installed()
    p.eng.set_sampling_correlation(M)
    assert p.eng.sampling_correlation_installed()
    p.eng.optimize(p.states)
    clipped = _check_samples(L, p, M, noise["trunc"], "injected %s %s" % (model, opt_name))
    assert clipped >= 1                                     # the bounds and M were chosen so that the clip is exercised
    # a transposed read would not have passed: the statement with M^T differs by far more than the bound
    sigma0 = CU.cem_sigma32(p.oracle()._init_mean(), p.oracle()._init_var(), p.lo_h, p.hi_h)
    wrong = CU.candidates64(M.T, noise["trunc"][0], sigma0, p.oracle()._init_mean(), p.lo_h, p.hi_h)[0]
    assert np.abs(wrong - p.eng.get_trace(0, L.TRACE_SAMPLES)).max() > 1e-2


# ---- 2. own draws: the kernel's Philox keying is the existing one ----------------------------------------------------
@pytest.mark.parametrize("model,opt_name", CASES)
def test_samples_follow_the_rule_with_own_draws(L, model, opt_name):
    p = Problem(L, model, opt_name, seed=7)
    M = _mix(1)
    p.eng.set_trace(True)
    p.eng.set_sampling_correlation(M)
    p.eng.optimize(p.states)
    z = [p.eng.dump_noise(L.NOISE_TRUNC_NORMAL, 0, it, (N, A, H, p.U)) for it in range(ITERS)]     # still the UNMIXED draws
    assert all(np.abs(zi).max() <= 2.0 for zi in z) and not np.array_equal(z[0], z[1])
    _check_samples(L, p, M, z, "own draws %s %s" % (model, opt_name))


# ---- 3. identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pendulum", "mlp"])
def test_identity_matrix_gives_the_uncorrelated_bits(L, monkeypatch, model):
    # Both handles on the per-iteration route, where the uncorrelated draw is candidate<SRC_TRUNC>'s expression and the refit
    # between the iterations is the same kernel: on the pendulum a traced handle without a matrix would otherwise stay on the
    # persistent kernel, whose PI2 refit sums in another order (its iteration-1 mean, hence its samples, differ in the last bit).
    monkeypatch.setenv("BBMPC_FUSED", "0")
    a, b = Problem(L, model, "PI2", seed=3), Problem(L, model, "PI2", seed=3)
    a.eng.set_trace(True)
    b.eng.set_trace(True)
    b.eng.set_sampling_correlation(np.eye(H, dtype=F))
    a.eng.optimize(a.states)
    b.eng.optimize(b.states)
    for it in range(ITERS):
        np.testing.assert_array_equal(b.eng.get_trace(it, L.TRACE_SAMPLES), a.eng.get_trace(it, L.TRACE_SAMPLES))


# ---- 4. lock-step control step ---------------------------------------------------------------------------------------
def _assert_rewards(p, got, want, samples):
    if p.model == "pendulum":
        np.testing.assert_allclose(got, want, rtol=R_RTOL, atol=R_ATOL)
    else:
        assert_cheetah_rewards(got, want, MLP_R_RTOL, MLP_R_ATOL, margin=lambda: cheetah_threshold_margin(p.ev, p.states, samples))


@pytest.mark.parametrize("model", ["pendulum", "mlp"])
def test_cem_control_step_in_lock_step(L, model):
    p = Problem(L, model, "CEM")
    M, noise = _mix(2), p.noise(2)
    p.eng.set_trace(True)
    p.eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    p.eng.set_sampling_correlation(M)
    act, nxt, rew = p.eng.optimize(p.states)
    hip_el = [p.eng.get_trace(it, L.TRACE_ELITES) for it in range(ITERS)]
    hip_r = [p.eng.get_trace(it, L.TRACE_REWARDS) for it in range(ITERS)]
    hip_s = [p.eng.get_trace(it, L.TRACE_SAMPLES) for it in range(ITERS)]
    # tie tolerance at the elite boundary: the rollout tolerance on the pendulum, twice that on the learned model
    # (tests/test_gpu_pendulum.py _cem_lockstep, tests/test_gpu_mlp.py _lockstep_select)
    rtol, atol, tie = (R_RTOL, R_ATOL, 1.0) if model == "pendulum" else (MLP_R_RTOL, MLP_R_ATOL, 2.0)

    def select(it, r_o, own):
        _assert_rewards(p, hip_r[it], r_o, hip_s[it])
        for a in range(A):
            he = hip_el[it][a]
            if set(own[a]) != set(he):
                kth = np.sort(r_o[:, a])[::-1][K - 1]
                for n in set(own[a]) ^ set(he):
                    assert abs(r_o[n, a] - kth) <= tie * (atol + rtol * abs(kth)), "elite sets differ beyond the tie tolerance"
            np.testing.assert_array_equal(he, O.topk_desc(hip_r[it][:, a], K))
        return hip_el[it]
    cem = p.oracle(M)
    cem._optimize(p.states, noise, forced_elites=select)
    m_atol, v_rtol, v_atol = (2e-5, 1e-5, 2e-5) if model == "pendulum" else (1e-4, 1e-4, 1e-4)
    for it in range(ITERS):
        np.testing.assert_allclose(hip_s[it], cem.trace[it]["samples"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(p.eng.get_trace(it, L.TRACE_MEAN), cem.trace[it]["mean"], rtol=0, atol=m_atol)
        np.testing.assert_allclose(p.eng.get_trace(it, L.TRACE_VAR), cem.trace[it]["var"], rtol=v_rtol, atol=v_atol)
        s = hip_s[it]
        assert s.min() >= p.lo[0] and s.max() <= p.hi[0]                            # the clipped candidates are what is stored
    np.testing.assert_allclose(act, cem.trace[-1]["mean"][:, 0], rtol=0, atol=m_atol)


@pytest.mark.parametrize("model", ["pendulum", "mlp"])
def test_pi2_control_step_in_lock_step(L, model):
    lam = 1.0 if model == "pendulum" else 5.0
    p = Problem(L, model, "PI2", lamda=lam)
    M = _mix(3)
    p.eng.set_trace(True)
    p.eng.set_sampling_correlation(M)
    pi2 = p.oracle(lamda=lam)
    m_atol = 2e-5 if model == "pendulum" else 1e-4
    for step in range(2):                                   # the second control step starts from the shifted mean
        noise = p.noise(10 + step)
        p.eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
        act, _, _ = p.eng.optimize(p.states)
        hip_r = [p.eng.get_trace(it, L.TRACE_REWARDS) for it in range(ITERS)]
        hip_s = [p.eng.get_trace(it, L.TRACE_SAMPLES) for it in range(ITERS)]

        def lock(it, r_o):
            if model == "pendulum":
                np.testing.assert_allclose(hip_r[it], r_o, rtol=R_RTOL, atol=R_ATOL)
            else:
                # (the indicator margins are those of the rolled-out, feasible samples; the penalty is common to both sides)
                _assert_rewards(p, hip_r[it], r_o, hip_s[it])
            return hip_r[it]
        act_o = pi2._optimize(p.states, CU.mixed_noise(M, noise), rewards_override=lock)
        for it in range(ITERS):
            np.testing.assert_allclose(hip_s[it], pi2.trace[it]["samples"], rtol=0, atol=2e-5)
            np.testing.assert_allclose(p.eng.get_trace(it, L.TRACE_MEAN), pi2.trace[it]["mean"], rtol=0, atol=m_atol)
        assert max(float(t["penalty"].max()) for t in pi2.trace) > 0.0          # mixed draws did leave the bounds: the penalty is live
        np.testing.assert_allclose(act, act_o, rtol=0, atol=m_atol)
        np.testing.assert_allclose(p.eng.get_state("prev_mean"), pi2.prev, rtol=0, atol=m_atol)


# ---- 5. particles on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["CEM", "PI2"])
def test_with_particles_on(L, opt_name):
    P = 5
    p = Problem(L, "mlp", opt_name)
    M, noise = _mix(4), p.noise(4)
    sigma = np.full(p.S, 0.02, F)
    eps = np.random.default_rng(5).standard_normal((A, P, H, p.S)).astype(F)
    p.eng.set_particles(P, sigma, 0.5)
    p.eng.inject_noise(L.NOISE_PROCESS, np.stack([eps] * ITERS))          # every iteration (and evaluate_particles) rolls the same eps
    p.eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    p.eng.set_trace(True)
    p.eng.set_sampling_correlation(M)
    act, nxt, rew = p.eng.optimize(p.states)
    assert np.all(np.isfinite(act)) and np.all(np.isfinite(nxt)) and np.all(np.isfinite(rew))
    _check_samples(L, p, M, noise["trunc"], "particles %s" % opt_name)
    if opt_name == "CEM":                                   # (PI2's scores carry the penalty, which evaluate_particles does not charge)
        for it in range(ITERS):
            samples = p.eng.get_trace(it, L.TRACE_SAMPLES)
            scores, _ = p.eng.evaluate_particles(p.states, samples)
            assert_cheetah_rewards(p.eng.get_trace(it, L.TRACE_REWARDS), scores, MLP_R_RTOL, MLP_R_ATOL, max_flip_frac=0.0)


# ---- 6. HIP-source reward on pendulum dynamics -----------------------------------------------------------------------
def test_with_a_hip_source_reward(L):
    from tests.test_gpu_user_functions import INTENDED_PENDULUM_REWARD
    from tests.test_gpu_user_functions import R_ATOL as U_ATOL, R_RTOL as U_RTOL
    p = Problem(L, "pendulum", "CEM", reward_source=INTENDED_PENDULUM_REWARD)
    M, noise = _mix(5), p.noise(5)
    p.eng.set_trace(True)
    p.eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    p.eng.set_sampling_correlation(M)
    p.eng.optimize(p.states)
    assert _check_samples(L, p, M, noise["trunc"], "HIP-source reward") >= 1
    for it in range(ITERS):
        samples = p.eng.get_trace(it, L.TRACE_SAMPLES)
        np.testing.assert_allclose(p.eng.get_trace(it, L.TRACE_REWARDS), p.eng.evaluate(p.states, samples), rtol=U_RTOL, atol=U_ATOL)
        ev = O.Evaluator(lambda cur, act, nxt: O.pendulum_reward(cur, act, nxt, as_executed=False), O.Handler(O.pendulum_dynamics, True))
        np.testing.assert_allclose(p.eng.get_trace(it, L.TRACE_REWARDS), ev(p.states, samples), rtol=U_RTOL, atol=U_ATOL)


# ---- 7. off switch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,opt_name", [("pendulum", "CEM"), ("mlp", "PI2")])
def test_removing_the_matrix_restores_every_path(L, model, opt_name):
    a, b = Problem(L, model, opt_name, seed=11), Problem(L, model, opt_name, seed=11)
    b.eng.set_sampling_correlation(_mix(6))
    b.eng.set_sampling_correlation(None)
    assert not b.eng.sampling_correlation_installed()
    sa = sb = a.states
    for t in range(3):
        ra, rb = a.eng.optimize(sa, t), b.eng.optimize(sb, t)
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)
        sa, sb = ra[1], rb[1]
    assert a.eng.call_stats() == b.eng.call_stats() and a.eng.graph_stats() == b.eng.graph_stats()
    for t in range(3, 9):                                   # ... and on into the steady state (the learned model's step graph)
        ra, rb = a.eng.optimize(sa, t), b.eng.optimize(sb, t)
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)
        sa, sb = ra[1], rb[1]
    assert a.eng.call_stats() == b.eng.call_stats() and a.eng.graph_stats() == b.eng.graph_stats()
    # installed after use and removed again: the next calls are again those of the untouched twin
    b.eng.set_sampling_correlation(_mix(6))
    b.eng.set_sampling_correlation(None)
    a.eng.reset()
    b.eng.reset()
    for x, y in zip(a.eng.optimize(a.states), b.eng.optimize(b.states)):
        np.testing.assert_array_equal(x, y)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def _pendulum_engine(L, opt, **kw):
    from blackbox_mpc_amd.engine import Engine
    return Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H,
                  population_size=N, max_iterations=ITERS, num_elite=K, seed=5, **kw)


def _refused(L, make, matrix, code, match):
    eng, twin = make(), make()
    with pytest.raises(L.BBMPCError, match=match) as ei:
        eng.set_sampling_correlation(matrix)
    assert ei.value.code == code
    assert not eng.sampling_correlation_installed()
    states = O.pendulum_start_states(A)
    for x, y in zip(eng.optimize(states), twin.optimize(states)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("opt_name", ["OPT_RANDOM_SEARCH", "OPT_PSO", "OPT_SPSA", "OPT_CMAES"])
def test_other_optimizers_are_refused(L, opt_name):
    _refused(L, lambda: _pendulum_engine(L, getattr(L, opt_name)), _mix(), L.E_UNSUPPORTED, "CEM or PI2")


@pytest.mark.parametrize("opt_name", ["OPT_CEM", "OPT_PI2"])
def test_a_sharded_population_is_refused(L, monkeypatch, opt_name):
    monkeypatch.setenv("BBMPC_POPSHARD_LOOPBACK", "2")      # one handle plays both shards: no communicator needed
    _refused(L, lambda: _pendulum_engine(L, getattr(L, opt_name)), _mix(), L.E_UNSUPPORTED, "sharded")


@pytest.mark.parametrize("opt_name", ["OPT_CEM", "OPT_PI2"])
def test_bad_matrices_are_refused(L, opt_name):
    make = lambda: _pendulum_engine(L, getattr(L, opt_name))          # noqa: E731
    _refused(L, make, np.zeros((H, H + 1), F), L.E_INVALID, "planning_horizon")
    _refused(L, make, np.zeros(H * H - 1, F), L.E_INVALID, "planning_horizon")
    for val in (np.nan, np.inf):
        bad = _mix()
        bad[3, 1] = val
        _refused(L, make, bad, L.E_INVALID, "non-finite")
    # a refused replacement leaves the installed matrix in use
    eng, twin = make(), make()
    eng.set_sampling_correlation(_mix(7))
    twin.set_sampling_correlation(_mix(7))
    with pytest.raises(L.BBMPCError):
        eng.set_sampling_correlation(np.full((H, H), np.nan, F))
    assert eng.sampling_correlation_installed()
    states = O.pendulum_start_states(A)
    for x, y in zip(eng.optimize(states), twin.optimize(states)):
        np.testing.assert_array_equal(x, y)
    # H * dim_u past the LDS tile
    from blackbox_mpc_amd.engine import Engine
    big = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_CHEETAH, [-1.0] * 8, [1.0] * 8, dim_s=18, num_agents=1, planning_horizon=80,
                 population_size=16, max_iterations=1, num_elite=4)
    with pytest.raises(L.BBMPCError, match="636") as ei:
        big.set_sampling_correlation(np.eye(80, dtype=F))
    assert ei.value.code == L.E_UNSUPPORTED


# ---- the Python surface ----------------------------------------------------------------------------------------------
def test_mpc_policy_passes_noise_beta_through(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.utils.colored_noise import colored_noise_mixing
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    act, obs = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    kw = dict(reward_function=pendulum_reward_function, env_action_space=act, env_observation_space=obs, true_model=True,
              dynamics_function=PendulumTrueModel(), num_agents=A, planning_horizon=H, population_size=N, max_iterations=ITERS, seed=9)
    for name, extra in (("CEM", dict(num_elite=K)), ("PI2", {})):
        pol = MPCPolicy(optimizer_name=name, noise_beta=2.0, **kw, **extra)
        eng = pol._optimizer._engine
        assert eng.sampling_correlation_installed()
        plain = MPCPolicy(optimizer_name=name, **kw, **extra)
        assert not plain._optimizer._engine.sampling_correlation_installed()
        eng.set_trace(True)
        states = O.pendulum_start_states(A)
        action, _, _ = pol.act(states, 0)
        assert action.shape == (A, 1) and np.all(np.abs(action) <= 2.0)
        p = Problem.__new__(Problem)                        # the samples are those of colored_noise_mixing(H, 2)
        p.eng, p.opt_name, p.U, p.lo, p.hi, p.ev = eng, name, 1, [-2.0], [2.0], None
        p.lo_h, p.hi_h = np.full((H, 1), -2.0, F), np.full((H, 1), 2.0, F)
        z = [eng.dump_noise(L.NOISE_TRUNC_NORMAL, 0, it, (N, A, H, 1)) for it in range(ITERS)]
        _check_samples(L, p, colored_noise_mixing(H, 2.0), z, "MPCPolicy %s" % name)
        assert not np.array_equal(action, plain.act(states, 0)[0])
