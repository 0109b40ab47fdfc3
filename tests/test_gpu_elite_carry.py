"""GPU tests of CEM's elite carry-over (bbmpc_set_elite_carry), through the C ABI, against the NumPy
statement of tests/elite_carry_util.py.

Shapes follow tests/test_gpu_correlated.py: N = 70 (the particle stride is 128, and with a matrix the correlated draw runs two
workgroups, the second partial), A = 2, H = 5, k = 8; 3 iterations, keep = 3, shift = 2; the analytic pendulum (U = 1) and that
file's tiny learned model (U = 5, so that j = t * U + u and the shift by U rows are exercised).  Injected noise and the
parity trace throughout.  The carried columns are compared bit for bit; everything else with the tolerances of
test_gpu_correlated.py's test_cem_control_step_in_lock_step."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import elite_carry_util as EC
from tests.test_gpu_correlated import MLP_R_ATOL, MLP_R_RTOL, TINY_MLP, A, H, K, N, _mix
from tests.parity_util import assert_cheetah_rewards, cheetah_threshold_margin
from tests.test_particles_cpu import R_ATOL, R_RTOL                   # pendulum H-step rewards: rtol 2e-4, atol 2e-3

pytestmark = pytest.mark.gpu
F = np.float32
ITERS, KEEP, SHIFT = 3, 3, 2
MODELS_MIX = [("pendulum", False), ("pendulum", True), ("mlp", False), ("mlp", True)]


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


class Problem:
    """A traced CEM handle with injected draws, optionally a mixing matrix, and the oracle that goes with it."""

    def __init__(self, L, model, with_mix=False, carry=(KEEP, SHIFT), reward_source=None, noise_seed=1, **kw):
        from blackbox_mpc_amd.engine import Engine
        self.L, self.model = L, model
        if model == "pendulum":
            self.lo, self.hi, self.S, self.U = [-2.0], [2.0], 3, 1
            rk = L.REW_USER if reward_source else L.REW_PENDULUM
            self.eng = Engine(L.OPT_CEM, L.DYN_PENDULUM, rk, self.lo, self.hi, dim_s=3, num_agents=A, planning_horizon=H,
                              population_size=N, max_iterations=ITERS, num_elite=K, **kw)
            if reward_source:
                self.eng.set_reward_source(reward_source)
            self.ev = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
            self.states = O.pendulum_start_states(A)
        else:
            from tests.test_gpu_mlp import _problem
            dims, acts, S, U, reward = TINY_MLP
            self.eng, self.ev, self.lo, self.hi = _problem(L, dims, acts, S, U, reward, True, A=A, H=H, opt=L.OPT_CEM, N=N,
                                                           iters=ITERS, k=K, **kw)
            self.S, self.U = S, U
            self.states = O.cheetah_start_states(A, S).astype(F)
        self.mix = _mix(8) if with_mix else None
        rng = np.random.default_rng(noise_seed)
        self.noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, self.U)) for _ in range(ITERS)]}
        self.eng.set_trace(True)
        self.eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(self.noise["trunc"]))
        if with_mix:
            self.eng.set_sampling_correlation(self.mix)
        if carry != (0, 0):
            self.eng.set_elite_carry(*carry)

    def oracle(self, keep=KEEP, shift=SHIFT):
        return EC.CarryCEM(self.ev, self.lo, self.hi, horizon=H, max_iterations=ITERS, population=N, num_elite=K, num_agents=A,
                           keep=keep, shift=shift, mix=self.mix)

    def step(self):
        """one control step; (outputs, per-iteration traces)"""
        L = self.L
        out = self.eng.optimize(self.states)
        tr = [dict(samples=self.eng.get_trace(it, L.TRACE_SAMPLES), rewards=self.eng.get_trace(it, L.TRACE_REWARDS),
                   elites=self.eng.get_trace(it, L.TRACE_ELITES), mean=self.eng.get_trace(it, L.TRACE_MEAN),
                   var=self.eng.get_trace(it, L.TRACE_VAR)) for it in range(ITERS)]
        return out, tr


def _assert_kept(tr, keep=KEEP):
    """iterations 1 ..: the last `keep` columns are the previous iteration's first `keep` traced elites, bit for bit"""
    for it in range(1, ITERS):
        prev, cur = tr[it - 1], tr[it]
        for a in range(A):
            assert np.all((prev["elites"][a] >= 0) & (prev["elites"][a] < N))
            np.testing.assert_array_equal(cur["samples"][N - keep:, a], prev["samples"][prev["elites"][a][:keep], a])


def _assert_shifted(last, first, shift=SHIFT):
    """`first` (iteration 0 of a control step) ends in the first `shift` elites of `last` (the last iteration of the control
    step before), rows 1 .. H-1 moved to 0 .. H-2 and row H-1 repeated, bit for bit"""
    for a in range(A):
        for e in range(shift):
            row = last["samples"][last["elites"][a][e], a]                    # [H,U]
            got = first["samples"][N - shift + e, a]
            np.testing.assert_array_equal(got[:H - 1], row[1:])
            np.testing.assert_array_equal(got[H - 1], row[H - 1])


# ---- 1. keep, bitwise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,with_mix", MODELS_MIX)
def test_kept_elites_are_the_last_columns_bit_for_bit(L, monkeypatch, model, with_mix):
    monkeypatch.setenv("BBMPC_FUSED", "0")                  # the twin without carry on the per-iteration route as well
    p, twin = Problem(L, model, with_mix), Problem(L, model, with_mix, carry=(0, 0))
    assert p.eng.elite_carry() == (KEEP, SHIFT, 0) and twin.eng.elite_carry() == (0, 0, 0)
    _, tr = p.step()
    _, tw = twin.step()
    _assert_kept(tr)
    # iteration 0 of the first control step: nothing stored, so no replaced column -- every column is the twin's
    np.testing.assert_array_equal(tr[0]["samples"], tw[0]["samples"])
    if model == "pendulum":                                 # lane-per-trajectory kernel: a carried row scores what it scored
        for it in range(1, ITERS):
            for a in range(A):
                prev = tr[it - 1]
                np.testing.assert_array_equal(tr[it]["rewards"][N - KEEP:, a], prev["rewards"][prev["elites"][a][:KEEP], a])


# ---- 2. shift, bitwise -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,with_mix", [("pendulum", False), ("mlp", True)])
def test_shifted_elites_open_the_next_control_step(L, model, with_mix):
    p = Problem(L, model, with_mix)
    assert p.eng.elite_carry()[2] == 0
    _, s0 = p.step()
    assert p.eng.elite_carry() == (KEEP, SHIFT, SHIFT)
    _, s1 = p.step()
    assert p.eng.elite_carry() == (KEEP, SHIFT, SHIFT)
    _assert_shifted(s0[-1], s1[0])
    # quirk Q2 and the same injected draws: the other columns of both first iterations are the same candidates, so
    # iteration 0 of step 0 had no replaced column (its last two are the draws, which step 1 overwrote)
    np.testing.assert_array_equal(s1[0]["samples"][:N - SHIFT], s0[0]["samples"][:N - SHIFT])
    assert not np.array_equal(s1[0]["samples"][N - SHIFT:], s0[0]["samples"][N - SHIFT:])
    _assert_kept(s0)
    _assert_kept(s1)


# ---- 3. lock step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,with_mix", MODELS_MIX)
def test_two_control_steps_in_lock_step(L, model, with_mix):
    p = Problem(L, model, with_mix, noise_seed=2)
    cem = p.oracle()
    # tie tolerance at the elite boundary: the rollout tolerance on the pendulum, twice that on the learned model
    rtol, atol, tie = (R_RTOL, R_ATOL, 1.0) if model == "pendulum" else (MLP_R_RTOL, MLP_R_ATOL, 2.0)
    m_atol, v_rtol, v_atol = (2e-5, 1e-5, 2e-5) if model == "pendulum" else (1e-4, 1e-4, 1e-4)
    for step in range(2):
        (act, _, _), tr = p.step()

        def select(it, r_o, own):
            if model == "pendulum":
                np.testing.assert_allclose(tr[it]["rewards"], r_o, rtol=R_RTOL, atol=R_ATOL)
            else:
                assert_cheetah_rewards(tr[it]["rewards"], r_o, MLP_R_RTOL, MLP_R_ATOL,
                                       margin=lambda: cheetah_threshold_margin(p.ev, p.states, tr[it]["samples"]))
            for a in range(A):
                he = tr[it]["elites"][a]
                if set(own[a]) != set(he):
                    kth = np.sort(r_o[:, a])[::-1][K - 1]
                    for n in set(own[a]) ^ set(he):
                        assert abs(r_o[n, a] - kth) <= tie * (atol + rtol * abs(kth)), "elite sets differ beyond the tie tolerance"
                np.testing.assert_array_equal(he, O.topk_desc(tr[it]["rewards"][:, a], K))
            return tr[it]["elites"]
        cem._optimize(p.states, p.noise, forced_elites=select)
        for it in range(ITERS):
            np.testing.assert_allclose(tr[it]["samples"], cem.trace[it]["samples"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(tr[it]["mean"], cem.trace[it]["mean"], rtol=0, atol=m_atol)
            np.testing.assert_allclose(tr[it]["var"], cem.trace[it]["var"], rtol=v_rtol, atol=v_atol)
        np.testing.assert_allclose(act, cem.trace[-1]["mean"][:, 0], rtol=0, atol=m_atol)
        np.testing.assert_array_equal(act, tr[-1]["mean"][:, 0])               # the action is the first step of the final mean
        assert p.eng.elite_carry()[2] == SHIFT and cem.stored.shape == (SHIFT, A, H, p.U)


# ---- 4. monotone best ------------------------------------------------------------------------------------------------
def test_the_best_reward_does_not_fall_with_one_kept_elite(L):
    p = Problem(L, "pendulum", carry=(1, 0), noise_seed=3)
    for step in range(2):
        _, tr = p.step()
        best = np.stack([t["rewards"].max(axis=0) for t in tr])               # [iters, A]
        print("best rewards per iteration:", best.tolist())
        for it in range(1, ITERS):
            assert np.all(best[it] >= best[it - 1] - (R_ATOL + R_RTOL * np.abs(best[it - 1])))
        assert p.eng.elite_carry() == (1, 0, 0)


# ---- 5. off is off ---------------------------------------------------------------------------------------------------
def _plain_engine(L, opt, k=K, **kw):
    from blackbox_mpc_amd.engine import Engine
    return Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H,
                  population_size=N, max_iterations=ITERS, num_elite=k, seed=5, **kw)


def test_switched_off_restores_the_default_route(L):
    a, b = _plain_engine(L, L.OPT_CEM), _plain_engine(L, L.OPT_CEM)
    states = O.pendulum_start_states(A)
    b.set_elite_carry(KEEP, SHIFT)
    for _ in range(2):                                      # b plans two control steps with carry, a without
        a.optimize(states)
        b.optimize(states)
    assert b.elite_carry() == (KEEP, SHIFT, SHIFT)
    b.set_elite_carry(0, 0)
    assert b.elite_carry() == (0, 0, 0)
    sa = sb = states
    for t in range(4):                                      # same control-step counters, same distribution (Q2): same bits
        ra, rb = a.optimize(sa, t), b.optimize(sb, t)
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)
        sa, sb = ra[1], rb[1]
    # a handle that never ran with it: also the same launches (resident / launched calls)
    c, d = _plain_engine(L, L.OPT_CEM), _plain_engine(L, L.OPT_CEM)
    d.set_elite_carry(KEEP, SHIFT)
    d.set_elite_carry(0, 0)
    for t in range(4):
        for x, y in zip(c.optimize(states, t), d.optimize(states, t)):
            np.testing.assert_array_equal(x, y)
    assert c.call_stats() == d.call_stats() and c.graph_stats() == d.graph_stats()


def test_switched_off_restores_every_traced_iteration(L, monkeypatch):
    monkeypatch.setenv("BBMPC_FUSED", "0")
    p, twin = Problem(L, "pendulum"), Problem(L, "pendulum", carry=(0, 0))
    p.step()
    twin.step()
    p.eng.set_elite_carry(0, 0)
    (act, nxt, rew), tr = p.step()
    (act_t, nxt_t, rew_t), tw = twin.step()
    for x, y in ((act, act_t), (nxt, nxt_t), (rew, rew_t)):
        np.testing.assert_array_equal(x, y)
    for it in range(ITERS):
        for key in ("samples", "rewards", "elites", "mean", "var"):
            np.testing.assert_array_equal(tr[it][key], tw[it][key])


# ---- 6. lifetime -----------------------------------------------------------------------------------------------------
def test_reset_drops_the_stored_elites_and_keeps_the_setting(L):
    p = Problem(L, "mlp")
    _, s0 = p.step()
    assert p.eng.elite_carry() == (KEEP, SHIFT, SHIFT)
    p.eng.reset()
    assert p.eng.elite_carry() == (KEEP, SHIFT, 0)
    _, s1 = p.step()
    np.testing.assert_array_equal(s1[0]["samples"], s0[0]["samples"])          # no replaced column: same noise, Q2
    _assert_kept(s1)                                                          # the setting survived
    assert p.eng.elite_carry() == (KEEP, SHIFT, SHIFT)
    # ... and so does an accepted call of the setter
    p.eng.set_elite_carry(KEEP, SHIFT)
    assert p.eng.elite_carry() == (KEEP, SHIFT, 0)
    _, s2 = p.step()
    np.testing.assert_array_equal(s2[0]["samples"], s0[0]["samples"])


@pytest.mark.parametrize("model", ["pendulum", "mlp"])
def test_other_calls_between_two_steps_leave_the_stored_elites_alone(L, model):
    p = Problem(L, model)
    _, s0 = p.step()
    rng = np.random.default_rng(9)
    seqs = rng.uniform(p.lo[0], p.hi[0], (N, A, H, p.U)).astype(F)
    assert np.all(np.isfinite(p.eng.evaluate(p.states, seqs)))
    ps, pr = p.eng.predict_trajectories(p.states, seqs[0])
    assert np.all(np.isfinite(ps)) and np.all(np.isfinite(pr))
    p.eng.set_trace(False)
    p.eng.set_trace(True)
    assert p.eng.elite_carry() == (KEEP, SHIFT, SHIFT)
    _, s1 = p.step()
    _assert_shifted(s0[-1], s1[0])
    np.testing.assert_array_equal(s1[0]["samples"][:N - SHIFT], s0[0]["samples"][:N - SHIFT])


# ---- 7. other evaluators ---------------------------------------------------------------------------------------------
def _assert_two_steps(p):
    _, s0 = p.step()
    _, s1 = p.step()
    _assert_kept(s0)
    _assert_kept(s1)
    _assert_shifted(s0[-1], s1[0])
    np.testing.assert_array_equal(s1[0]["samples"][:N - SHIFT], s0[0]["samples"][:N - SHIFT])
    for t in s0 + s1:
        assert np.all(np.isfinite(t["rewards"]))


def test_with_particles_on(L):
    p = Problem(L, "pendulum")
    p.eng.set_particles(4, np.full(3, 0.02, F), 0.5)
    _assert_two_steps(p)


def test_with_a_hip_source_reward(L):
    from tests.test_gpu_user_functions import INTENDED_PENDULUM_REWARD
    _assert_two_steps(Problem(L, "pendulum", reward_source=INTENDED_PENDULUM_REWARD))


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def _refused(L, eng, keep, shift, code, match):
    before = eng.elite_carry()
    with pytest.raises(L.BBMPCError, match=match) as ei:
        eng.set_elite_carry(keep, shift)
    assert ei.value.code == code
    assert eng.elite_carry() == before


@pytest.mark.parametrize("opt_name", ["OPT_RANDOM_SEARCH", "OPT_PI2", "OPT_PSO", "OPT_SPSA", "OPT_CMAES"])
def test_other_optimizers_are_refused(L, opt_name):
    eng = _plain_engine(L, getattr(L, opt_name))
    _refused(L, eng, KEEP, SHIFT, L.E_UNSUPPORTED, "CEM")
    assert eng.elite_carry() == (0, 0, 0)
    eng.set_elite_carry(0, 0)                               # switching off what is off is no refusal
    act, nxt, rew = eng.optimize(O.pendulum_start_states(A))
    assert np.all(np.isfinite(act))


def test_a_sharded_population_is_refused(L, monkeypatch):
    monkeypatch.setenv("BBMPC_POPSHARD_LOOPBACK", "2")      # one handle plays both shards: no communicator needed
    eng = _plain_engine(L, L.OPT_CEM)
    _refused(L, eng, KEEP, SHIFT, L.E_UNSUPPORTED, "sharded")
    assert eng.elite_carry() == (0, 0, 0)


def test_bad_counts_are_refused_and_leave_the_handle_as_it_was(L):
    p = Problem(L, "pendulum")
    _, s0 = p.step()
    assert p.eng.elite_carry() == (KEEP, SHIFT, SHIFT)
    _refused(L, p.eng, K + 1, SHIFT, L.E_INVALID, "num_elite")
    _refused(L, p.eng, KEEP, K + 1, L.E_INVALID, "num_elite")
    _refused(L, p.eng, KEEP, -1, L.E_INVALID, "negative")
    _refused(L, p.eng, -1, 0, L.E_INVALID, "negative")
    assert p.eng.elite_carry() == (KEEP, SHIFT, SHIFT)       # the earlier setting and its stored elites
    _, s1 = p.step()
    _assert_shifted(s0[-1], s1[0])                           # ... which the next control step still injects
    _assert_kept(s1)
    # keep = N on a handle whose num_elite is N: within num_elite, but no column would be left to draw
    full = _plain_engine(L, L.OPT_CEM, k=N)
    _refused(L, full, N, 0, L.E_INVALID, "population_size")
    _refused(L, full, 0, N, L.E_INVALID, "population_size")


# ---- 9. the Python surface -------------------------------------------------------------------------------------------
def test_mpc_policy_passes_the_arguments_through(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    act, obs = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    pol = MPCPolicy(optimizer_name="CEM", noise_beta=2.0, keep_elites=KEEP, shift_elites=SHIFT, reward_function=pendulum_reward_function,
                    env_action_space=act, env_observation_space=obs, true_model=True, dynamics_function=PendulumTrueModel(),
                    num_agents=A, planning_horizon=H, population_size=N, max_iterations=ITERS, num_elite=K, seed=9)
    eng = pol._optimizer._engine
    assert eng.elite_carry() == (KEEP, SHIFT, 0) and eng.sampling_correlation_installed()
    states = O.pendulum_start_states(A)
    for t in range(4):
        action, nxt, _ = pol.act(states, t)
        assert action.shape == (A, 1) and np.all(np.isfinite(action)) and np.all(np.abs(action) <= 2.0)
        states = nxt
    assert eng.elite_carry() == (KEEP, SHIFT, SHIFT)
    with pytest.raises(TypeError):
        MPCPolicy(optimizer_name="PI2", keep_elites=1, reward_function=pendulum_reward_function, env_action_space=act,
                  env_observation_space=obs, true_model=True, dynamics_function=PendulumTrueModel(), num_agents=A,
                  planning_horizon=H, population_size=N, max_iterations=ITERS)
