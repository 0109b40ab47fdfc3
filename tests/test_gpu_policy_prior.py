"""GPU tests of the learned policy prior (bbmpc_set_policy_prior_mlp, k_policy_prior_rollout) through
the C ABI, against the float64 statement of tests/policy_prior_util.py.

pi on rows and the rollouts are compared at tests/reward_mlp_util's one-step tolerance (rtol 2e-5 + atol 2e-5, the project's
single-Dense-stack tolerance).  The rollouts are checked TEACHER-FORCED: for every step the statement recomputes a_t from the
device's own s_t and the injected xi, and s_{t+1} from the device's own s_t and a_t, so each comparison spans one stack (the
clip is 1-Lipschitz and needs no margin) and no tolerance compounds.  Inside a control step the policy columns are compared
with bbmpc_predict_policy_rollouts bit for bit -- the same kernel, the same instantiation.

Shapes: K in {1, 16, 17} (one row, a full tile, a tile edge), H in {1, 5}, A in {1, 2}, N = 64, (S, U) in {(3, 1), (20, 6)},
policy widths 8, 24 and 200, one swish layer, one network at the limits (8 layers of 512)."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import elite_carry_util as EC
from tests import policy_prior_util as PP
from tests import reward_mlp_util as R
from tests import terminal_value_util as V
from tests.parity_util import assert_cheetah_rewards, cheetah_threshold_margin
from tests.test_gpu_correlated import MLP_R_ATOL, MLP_R_RTOL, TINY_MLP, _mix
from tests.test_gpu_mlp import CHEETAH, _problem
from tests.test_gpu_terminal_value import _dynamics, _engine, _raises, _set, _states

pytestmark = pytest.mark.gpu
F = np.float32
N, A2, H5, ITERS, K_EL = 64, 2, 5, 3, 8
KEEP, SHIFT = 3, 2
PEND_SPEC = ([4, 21, 24, 3], ["sigmoid", "tanh", None], 3, 1, "pendulum")      # hidden widths that are no multiple of 16


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _cem(L, spec, A, H, **kw):
    dims, acts, S, U, reward = spec
    eng, ev, lo, hi = _problem(L, dims, acts, S, U, reward, True, A=A, H=H, opt=L.OPT_CEM, N=N, iters=ITERS, k=K_EL, **kw)
    return eng, ev, lo, hi


def _start(A, S, seed=5):
    return np.random.default_rng(seed).normal(0, 0.5, (A, S)).astype(F)


# ---- 1. pi on rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("su", [(3, 1), (20, 6)], ids=["3-1", "20-6"])
def test_rows_against_the_statement(L, su):
    S, U = su
    eng, _, _, _ = _cem(L, PEND_SPEC if S == 3 else CHEETAH, 1, 1)
    assert "bbmpc_set_policy_prior_mlp" in _raises(L, L.E_STATE, lambda: eng.evaluate_policy_prior(np.zeros((1, S), F)))
    rt, at = R.ONE_STEP
    rng = np.random.default_rng(S)
    nets = PP.small_policies(S, U) + [PP.wide_policy(S, U)] + ([PP.limits_policy(S, U)] if S == 20 else [])
    for net in nets:
        net.install(eng, 3, 0.5)                               # (count and noise play no part in the rows call)
        for b in (1, 16, 17, 37):
            s = rng.normal(0, 0.7, (b, S)).astype(F)
            want = net(s)
            got = eng.evaluate_policy_prior(s)
            print(net.name, b, "max |pi - statement| = %.3g" % np.max(np.abs(got - want)))
            np.testing.assert_allclose(got, want, rtol=rt, atol=at)
        assert 0.1 < np.std(want) < 10


# ---- 2. the rollouts, teacher-forced ---------------------------------------------------------------------------------------
def _teacher_forced(pol, handler, states, xi, sigma, lo, hi, acts, sts):
    """acts [K,A,H,U], sts [K,A,H,S] from the device: every step recomputed from the device's own s_t (and a_t)"""
    K, A, H, U = acts.shape
    rt, at = R.ONE_STEP
    s_prev = np.concatenate([np.broadcast_to(states[None, :, None], (K, A, 1, states.shape[1])), sts[:, :, :-1]], axis=2)
    rows = s_prev.reshape(K * A * H, -1)
    a_want = PP.policy_action64(pol, rows, np.asarray(xi).transpose(1, 0, 2, 3).reshape(K * A * H, U), sigma, lo, hi)
    s_want = PP.model_step64(handler, rows, acts.reshape(K * A * H, U))
    print(pol.name, acts.shape, "max |a - statement| = %.3g, max |s' - statement| = %.3g"
          % (np.max(np.abs(acts.reshape(-1, U) - a_want)), np.max(np.abs(sts.reshape(s_want.shape) - s_want))))
    np.testing.assert_allclose(acts.reshape(-1, U), a_want, rtol=rt, atol=at)
    np.testing.assert_allclose(sts.reshape(s_want.shape), s_want, rtol=rt, atol=at)
    assert np.all(acts >= np.asarray(lo, F)) and np.all(acts <= np.asarray(hi, F))


ROLLOUT_CASES = [((3, 1), 1, 1, 1, 0), ((3, 1), 17, 5, 2, 1), ((3, 1), 16, 5, 1, 3), ((20, 6), 16, 5, 1, 2), ((20, 6), 17, 5, 2, 3),
                 ((20, 6), 1, 1, 2, 4), ((20, 6), 17, 1, 1, 1), ((20, 6), 17, 5, 2, 4)]


@pytest.mark.parametrize("su,K,H,A,pi", ROLLOUT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_rollouts_teacher_forced(L, su, K, H, A, pi):
    S, U = su
    eng, ev, lo, hi = _cem(L, PEND_SPEC if S == 3 else CHEETAH, A, H)
    pol = (PP.small_policies(S, U) + [PP.wide_policy(S, U)])[pi]
    sigma = 0.4
    pol.install(eng, K, sigma)
    assert eng.policy_prior() == (K, pytest.approx(sigma))
    states = _start(A, S)
    xi = np.random.default_rng(K + H).standard_normal((A, K, H, U)).astype(F)
    acts, sts = eng.predict_policy_rollouts(states, xi)
    _teacher_forced(pol, ev.handler, states, xi, sigma, lo, hi, acts, sts)
    clipped = np.mean((acts == -1.0) | (acts == 1.0))
    if K * H * A * U >= 80:
        assert 0.0 < clipped < 0.9                              # some actions sit on a bound, most do not
    # either output alone, and both NULL refused
    np.testing.assert_array_equal(eng.predict_policy_rollouts(states, xi, want_states=False)[0], acts)
    np.testing.assert_array_equal(eng.predict_policy_rollouts(states, xi, want_actions=False)[1], sts)
    assert L.lib.bbmpc_predict_policy_rollouts(eng._h, L.ptr(states), L.ptr(xi), None, None) == L.E_INVALID
    # the model step is what bbmpc_predict_next_state computes, at the one-step tolerance of two kernels
    cur = np.concatenate([np.broadcast_to(states[None, :, None], (K, A, 1, S)), sts[:, :, :-1]], axis=2).reshape(-1, S)
    nxt = eng.predict_next_state(np.ascontiguousarray(cur), acts.reshape(-1, U))
    np.testing.assert_allclose(sts.reshape(-1, S), nxt, rtol=2 * R.ONE_STEP[0], atol=2 * R.ONE_STEP[1])


def test_rollouts_at_the_limits_and_deterministic_policy(L):
    S, U, K, H, A = 20, 6, 17, 5, 2
    eng, ev, lo, hi = _cem(L, CHEETAH, A, H)
    states = _start(A, S)
    pol = PP.limits_policy(S, U)                               # 8 layers of 512: 16 waves, the LDS attribute raised
    pol.install(eng, K, 0.2)
    xi = np.random.default_rng(3).standard_normal((A, K, H, U)).astype(F)
    acts, sts = eng.predict_policy_rollouts(states, xi)
    _teacher_forced(pol, ev.handler, states, xi, 0.2, lo, hi, acts, sts)
    # sigma = 0 with K = 1: the deterministic policy rollout, whatever the noise
    pol = PP.small_policies(S, U)[3]
    pol.install(eng, 1, 0.0)
    a0, s0 = eng.predict_policy_rollouts(states, xi[:, :1])
    a1, s1 = eng.predict_policy_rollouts(states)
    np.testing.assert_array_equal(a0, a1)
    np.testing.assert_array_equal(s0, s1)
    _teacher_forced(pol, ev.handler, states, np.zeros((A, 1, H, U), F), 0.0, lo, hi, a0, s0)


# ---- 3. stream 12 ----------------------------------------------------------------------------------------------------------
def test_policy_noise_matches_the_documented_scheme(L):
    S, U, K, H, A = 3, 1, 17, 5, 2
    seed = 0x1234567890ABCDEF
    eng = _engine(L, "builtin", A=A, H=H, opt=L.OPT_CEM, population_size=N, max_iterations=ITERS, num_elite=K_EL, seed=seed,
                  agent_offset=5, num_agents_global=8)
    with pytest.raises(L.BBMPCError) as ei:
        eng.dump_noise(L.NOISE_POLICY, 0, 0, (A, K, H, U))
    assert ei.value.code == L.E_STATE
    pol = PP.small_policies(S, U)[1]
    pol.install(eng, K, 0.3)
    before = eng.dump_noise(L.NOISE_TRUNC_NORMAL, 0, 1, (N, A, H, U))
    for step, it in [(0, 0), (3, 1)]:
        got = eng.dump_noise(L.NOISE_POLICY, step, it, (A, K, H, U))
        want = PP.policy_noise_np(seed, step, it, A, K, H, U, agent_offset=5)
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)          # test_gpu_particles.py's process-noise tolerance
    with pytest.raises(L.BBMPCError):
        eng.dump_noise(L.NOISE_POLICY, 0, 0, (A, K, H + 1, U))
    # NULL noise = the handle's stream at the current control step, iteration 0
    states = _start(A, S)
    own = eng.predict_policy_rollouts(states)
    fed = eng.predict_policy_rollouts(states, eng.dump_noise(L.NOISE_POLICY, 0, 0, (A, K, H, U)))
    for x, y in zip(own, fed):
        np.testing.assert_array_equal(x, y)
    # injected noise is what the rollouts use
    xi = np.random.default_rng(1).standard_normal((ITERS, A, K, H, U)).astype(F)
    eng.inject_noise(L.NOISE_POLICY, xi)
    for x, y in zip(eng.predict_policy_rollouts(states), eng.predict_policy_rollouts(states, xi[0])):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(eng.predict_policy_rollouts(states)[0], own[0])
    with pytest.raises(L.BBMPCError) as ei:
        eng.inject_noise(L.NOISE_POLICY, xi[0])
    assert ei.value.code == L.E_INVALID
    eng.inject_noise(L.NOISE_POLICY, None)
    np.testing.assert_array_equal(eng.predict_policy_rollouts(states)[0], own[0])
    # the candidate draws are keyed as before
    np.testing.assert_array_equal(eng.dump_noise(L.NOISE_TRUNC_NORMAL, 0, 1, (N, A, H, U)), before)


# ---- 4. the control step ---------------------------------------------------------------------------------------------------
class Problem:
    """A traced CEM handle on test_gpu_correlated.py's tiny learned model (S = 18, U = 5) with injected draws, optionally a
    mixing matrix, carry and the prior, and the oracle that goes with it."""

    def __init__(self, L, with_mix=False, carry=(0, 0), prior=True, K=17, sigma=0.3, noise_seed=1, **kw):
        dims, acts, S, U, reward = TINY_MLP
        self.L, self.S, self.U, self.K, self.sigma, self.carry = L, S, U, K, sigma, carry
        self.eng, self.ev, self.lo, self.hi = _problem(L, dims, acts, S, U, reward, True, A=A2, H=H5, opt=L.OPT_CEM, N=N,
                                                       iters=ITERS, k=K_EL, **kw)
        self.states = O.cheetah_start_states(A2, S).astype(F)
        self.mix = _mix(8) if with_mix else None
        self.pol = PP.small_policies(S, U)[3]
        rng = np.random.default_rng(noise_seed)
        self.noise = {"trunc": [O.truncated_normal_noise(rng, (N, A2, H5, U)) for _ in range(ITERS)],
                      "policy": [rng.standard_normal((A2, K, H5, U)).astype(F) for _ in range(ITERS)]}
        self.eng.set_trace(True)
        self.eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(self.noise["trunc"]))
        if with_mix:
            self.eng.set_sampling_correlation(self.mix)
        if carry != (0, 0):
            self.eng.set_elite_carry(*carry)
        if prior:
            self.pol.install(self.eng, K, sigma)
            self.eng.inject_noise(L.NOISE_POLICY, np.stack(self.noise["policy"]))

    def step(self):
        L = self.L
        out = self.eng.optimize(self.states)
        tr = [dict(samples=self.eng.get_trace(it, L.TRACE_SAMPLES), rewards=self.eng.get_trace(it, L.TRACE_REWARDS),
                   elites=self.eng.get_trace(it, L.TRACE_ELITES), mean=self.eng.get_trace(it, L.TRACE_MEAN),
                   var=self.eng.get_trace(it, L.TRACE_VAR)) for it in range(ITERS)]
        return out, tr

    def columns(self, step):
        """per iteration (first policy column, carried columns)"""
        keep, shift = self.carry
        return [(N - c - self.K, c) for c in [shift if step > 0 else 0] + [keep] * (ITERS - 1)]


@pytest.mark.parametrize("with_mix", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("carry", [(0, 0), (KEEP, SHIFT)], ids=["nocarry", "carry"])
def test_control_step_columns_bit_for_bit(L, monkeypatch, with_mix, carry):
    monkeypatch.setenv("BBMPC_FUSED", "0")
    p = Problem(L, with_mix, carry)
    twin = Problem(L, with_mix, carry, prior=False)
    probe = Problem(L, prior=True)                              # a handle that only serves bbmpc_predict_policy_rollouts
    last = None
    for step in range(2):
        _, tr = p.step()
        _, tw = twin.step()
        for it, (col0, c) in enumerate(p.columns(step)):
            want = probe.eng.predict_policy_rollouts(p.states, p.noise["policy"][it], want_states=False)[0]
            np.testing.assert_array_equal(tr[it]["samples"][col0:col0 + p.K], want)
            assert np.all(np.isfinite(tr[it]["rewards"]))
            if it >= 1 and c:                                   # section 8h: the previous iteration's first elites, last columns
                for a in range(A2):
                    np.testing.assert_array_equal(tr[it]["samples"][N - c:, a], tr[it - 1]["samples"][tr[it - 1]["elites"][a][:c], a])
            if it == 0 and c:                                   # ... and the shifted elites of the control step before
                np.testing.assert_array_equal(tr[0]["samples"][N - c:],
                                              EC.shift_rows(EC.gather_elites(last["samples"], last["elites"], c)))
        # iteration 0 samples from the constructor distribution on both handles (quirk Q2): every column that is neither
        # the policy's nor carried is the twin's, bit for bit
        col0, c = p.columns(step)[0]
        np.testing.assert_array_equal(tr[0]["samples"][:col0], tw[0]["samples"][:col0])
        assert not np.array_equal(tr[0]["samples"][col0:col0 + p.K], tw[0]["samples"][col0:col0 + p.K])
        last = tr[-1]


@pytest.mark.parametrize("with_mix,carry", [(False, (0, 0)), (True, (KEEP, SHIFT))], ids=["plain", "mix-carry"])
def test_two_control_steps_in_lock_step(L, with_mix, carry):
    p = Problem(L, with_mix, carry, noise_seed=2)
    probe = Problem(L, prior=True)
    cem = PP.PriorCEM(p.ev, p.lo, p.hi, horizon=H5, max_iterations=ITERS, population=N, num_elite=K_EL, num_agents=A2,
                      count=p.K, keep=carry[0], shift=carry[1], mix=p.mix,
                      rollouts=lambda state, xi: probe.eng.predict_policy_rollouts(state, xi, want_states=False)[0])
    rtol, atol, tie = MLP_R_RTOL, MLP_R_ATOL, 2.0               # test_gpu_elite_carry.py's lock-step test, learned model
    for step in range(2):
        (act, _, _), tr = p.step()

        def select(it, r_o, own):
            assert_cheetah_rewards(tr[it]["rewards"], r_o, MLP_R_RTOL, MLP_R_ATOL,
                                   margin=lambda: cheetah_threshold_margin(p.ev, p.states, tr[it]["samples"]))
            for a in range(A2):
                he = tr[it]["elites"][a]
                if set(own[a]) != set(he):
                    kth = np.sort(r_o[:, a])[::-1][K_EL - 1]
                    for n in set(own[a]) ^ set(he):
                        assert abs(r_o[n, a] - kth) <= tie * (atol + rtol * abs(kth)), "elite sets differ beyond the tie tolerance"
                np.testing.assert_array_equal(he, O.topk_desc(tr[it]["rewards"][:, a], K_EL))
            return tr[it]["elites"]
        cem._optimize(p.states, p.noise, forced_elites=select)
        assert cem.columns == p.columns(step)
        for it in range(ITERS):
            np.testing.assert_allclose(tr[it]["samples"], cem.trace[it]["samples"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(tr[it]["mean"], cem.trace[it]["mean"], rtol=0, atol=1e-4)
            np.testing.assert_allclose(tr[it]["var"], cem.trace[it]["var"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(act, cem.trace[-1]["mean"][:, 0], rtol=0, atol=1e-4)
        np.testing.assert_array_equal(act, tr[-1]["mean"][:, 0])


# ---- 5. composition --------------------------------------------------------------------------------------------------------
def _composed(L, kind, K=17, H=5, A=2):
    """test_gpu_terminal_value.py's DYN_MLP handle (S = 3, U = 1, hidden 24) as a traced CEM handle with the prior"""
    eng = _engine(L, kind, A=A, H=H, opt=L.OPT_CEM, population_size=N, max_iterations=ITERS, num_elite=K_EL)
    pol = PP.small_policies(3, 1)[1]
    pol.install(eng, K, 0.3)
    eng.set_trace(True)
    return eng, pol


def _assert_policy_columns_scored(L, eng, K, H, rtol, atol):
    states = _states(2)
    eng.optimize(states)
    for it in range(ITERS):
        samples, rewards = eng.get_trace(it, L.TRACE_SAMPLES), eng.get_trace(it, L.TRACE_REWARDS)
        cols = samples[N - K:]
        assert np.all(np.abs(cols) <= 1.0) and np.all(np.isfinite(rewards))
        want = eng.evaluate(states, np.ascontiguousarray(cols))
        print("iteration", it, "max |traced - evaluate| = %.3g" % np.max(np.abs(rewards[N - K:] - want)))
        np.testing.assert_allclose(rewards[N - K:], want, rtol=rtol, atol=atol)


def test_with_a_reward_mlp_and_a_terminal_value(L):
    eng, _ = _composed(L, "mlp")
    _set(eng, V.small_nets()[1], 0.7)
    # test_gpu_terminal_value.py's evaluate tolerance: H-step rewards plus the terminal term
    _assert_policy_columns_scored(L, eng, 17, 5, R.H_STEP_RTOL, R.H_STEP_ATOL_PER_STEP * 5)


def test_with_a_hip_source_reward(L):
    eng, _ = _composed(L, "user")
    _assert_policy_columns_scored(L, eng, 17, 5, R.H_STEP_RTOL, R.H_STEP_ATOL_PER_STEP * 5)


def test_with_particles_on_a_plain_model(L):
    eng, _ = _composed(L, "builtin")
    P = 4
    eng.set_particles(P, np.full(3, 0.02, F), 0.5)
    eps = np.random.default_rng(7).standard_normal((2, P, 5, 3)).astype(F)
    eng.inject_noise(L.NOISE_PROCESS, np.stack([eps] * ITERS))        # every iteration and bbmpc_evaluate roll the same eps
    _assert_policy_columns_scored(L, eng, 17, 5, R.H_STEP_RTOL, R.H_STEP_ATOL_PER_STEP * 5)


# ---- 6. the off switch -----------------------------------------------------------------------------------------------------
def test_switched_off_restores_every_traced_iteration(L, monkeypatch):
    monkeypatch.setenv("BBMPC_FUSED", "0")
    p, twin = Problem(L, carry=(KEEP, SHIFT)), Problem(L, carry=(KEEP, SHIFT), prior=False)
    p.step()
    twin.step()
    p.eng.set_policy_prior_mlp(None, None, None)               # n_layers = 0
    assert _raises(L, L.E_STATE, p.eng.policy_prior)
    p.eng.reset()
    twin.eng.reset()                                           # (the stored elites of the two differ: both start again)
    (act, nxt, rew), tr = p.step()
    (act_t, nxt_t, rew_t), tw = twin.step()
    for x, y in ((act, act_t), (nxt, nxt_t), (rew, rew_t)):
        np.testing.assert_array_equal(x, y)
    for it in range(ITERS):
        for key in ("samples", "rewards", "elites", "mean", "var"):
            np.testing.assert_array_equal(tr[it][key], tw[it][key])


def test_switched_off_restores_the_default_route(L):
    dims, acts, S, U, reward = CHEETAH
    mk = lambda: _problem(L, dims, acts, S, U, reward, True, A=1, H=H5, opt=L.OPT_CEM, N=N, iters=ITERS, k=K_EL, seed=5)[0]
    c, d = mk(), mk()
    pol = PP.small_policies(S, U)[1]
    pol.install(d, 3, 0.1)
    states = O.cheetah_start_states(1, S).astype(F)
    plain, with_prior = c.optimize(states, 0), d.optimize(states, 0)       # one control step each, d with the prior
    assert not np.array_equal(plain[0], with_prior[0])
    d.set_policy_prior_mlp(None, None, None)
    d.set_policy_prior_mlp(None, None, None)                   # switching off what is off is no refusal
    for t in range(1, 7):                                      # same control-step counters, same distribution (Q2): same bits
        for x, y in zip(c.optimize(states, t), d.optimize(states, t)):
            np.testing.assert_array_equal(x, y)
    # a handle that never ran with it: also the same launches (graph replays, resident / launched calls)
    c, d = mk(), mk()
    pol.install(d, 3, 0.1)
    d.set_policy_prior_mlp(None, None, None)
    for t in range(6):
        for x, y in zip(c.optimize(states, t), d.optimize(states, t)):
            np.testing.assert_array_equal(x, y)
    assert c.call_stats() == d.call_stats() and c.graph_stats() == d.graph_stats()


# ---- 7. determinism --------------------------------------------------------------------------------------------------------
def test_two_runs_and_an_agent_split_give_equal_bits(L):
    dims, acts, S, U, reward = TINY_MLP
    K = 17
    pol = PP.small_policies(S, U)[3]
    states = O.cheetah_start_states(4, S).astype(F)

    def run(A, off):
        eng = _problem(L, dims, acts, S, U, reward, True, A=A, H=H5, opt=L.OPT_CEM, N=N, iters=ITERS, k=K_EL, seed=11,
                       agent_offset=off, num_agents_global=4)[0]
        pol.install(eng, K, 0.3)
        eng.set_trace(True)
        st = states[off:off + A]
        roll = eng.predict_policy_rollouts(st)                 # the handle's own stream 12
        out = eng.optimize(st)
        return roll, out, [eng.get_trace(it, L.TRACE_SAMPLES) for it in range(ITERS)]
    whole, again = run(4, 0), run(4, 0)
    lo, hi = run(2, 0), run(2, 2)
    for x, y in zip(whole[0] + whole[1] + tuple(whole[2]), again[0] + again[1] + tuple(again[2])):
        np.testing.assert_array_equal(x, y)
    for i in range(2):
        np.testing.assert_array_equal(whole[0][i], np.concatenate([lo[0][i], hi[0][i]], axis=1))
    for i in range(3):
        np.testing.assert_array_equal(whole[1][i], np.concatenate([lo[1][i], hi[1][i]], axis=0))
    for it in range(ITERS):
        np.testing.assert_array_equal(whole[2][it], np.concatenate([lo[2][it], hi[2][it]], axis=1))


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def _install_raw(L, eng, pol, count=3, std=0.1, dims=None, acts=None, stats="own", n_layers=None):
    """bbmpc_set_policy_prior_mlp through ctypes with any argument replaced; returns the status code"""
    import ctypes
    n = len(pol.ws) if n_layers is None else n_layers
    dims = list(pol.dims) if dims is None else dims
    acts = pol.codes() if acts is None else acts
    dims_a = (ctypes.c_int32 * len(dims))(*dims)
    acts_a = (ctypes.c_int32 * len(acts))(*acts)
    wp = (ctypes.c_void_p * len(pol.ws))(*[w.ctypes.data for w in pol.ws])
    bp = (ctypes.c_void_p * len(pol.bs))(*[b.ctypes.data for b in pol.bs])
    st = pol.stats if stats == "own" else stats
    sp = (ctypes.c_void_p * 4)(*[s.ctypes.data for s in st]) if st is not None else None
    return L.lib.bbmpc_set_policy_prior_mlp(eng._h, n, dims_a, acts_a, wp, bp, 1 if (st is not None or stats is None and pol.stats is not None) else 0,
                                            sp, count, ctypes.c_float(std))


def test_invalid_arguments_leave_the_handle_as_it_was(L):
    S, U = 3, 1
    eng, _, _, _ = _cem(L, PEND_SPEC, 1, H5)
    good, other = PP.small_policies(S, U)[1], PP.small_policies(S, U)[2]
    good.install(eng, 3, 0.25)
    states = _start(1, S)
    ref = eng.predict_policy_rollouts(states)
    E = L.E_INVALID
    assert _install_raw(L, eng, other, dims=[S + 1, 24, U]) == E
    assert _install_raw(L, eng, other, dims=[S, 24, U + 1]) == E
    assert _install_raw(L, eng, other, dims=[S, 0, U]) == E
    assert _install_raw(L, eng, other, acts=[99, 0]) == E
    assert _install_raw(L, eng, good, stats=None) == E                       # is_normalized without stats
    assert _install_raw(L, eng, other, std=-0.5) == E
    assert _install_raw(L, eng, other, std=float("nan")) == E
    assert _install_raw(L, eng, other, std=float("inf")) == E
    assert _install_raw(L, eng, other, count=0) == E
    assert _install_raw(L, eng, other, count=N) == E
    assert L.lib.bbmpc_set_policy_prior_mlp(eng._h, 2, None, None, None, None, 0, None, 3, 0.1) == E
    assert _install_raw(L, eng, other, n_layers=9, dims=[S] + [8] * 8 + [U], acts=[0] * 9) == L.E_UNSUPPORTED
    assert _install_raw(L, eng, other, dims=[S, 513, U]) == L.E_UNSUPPORTED
    assert eng.policy_prior() == (3, 0.25)
    for x, y in zip(ref, eng.predict_policy_rollouts(states)):
        np.testing.assert_array_equal(x, y)
    # count + max(keep, shift) >= population_size, in both orders
    eng.set_elite_carry(KEEP, SHIFT)
    assert _install_raw(L, eng, other, count=N - KEEP) == E
    assert _install_raw(L, eng, other, count=N - KEEP - 1) == 0
    eng.set_elite_carry(0, 0)
    eng.set_elite_carry(KEEP, SHIFT)                           # 60 + 3 < 64
    eng.set_elite_carry(0, 0)
    with pytest.raises(L.BBMPCError, match="policy prior") as ei:
        eng.set_elite_carry(KEEP + 1, SHIFT)
    assert ei.value.code == E and eng.elite_carry() == (0, 0, 0)
    assert np.all(np.isfinite(eng.optimize(states)[0]))
    # bbmpc_reset keeps the setting
    eng.reset()
    assert eng.policy_prior()[0] == N - KEEP - 1


def test_calls_without_a_network_are_state_errors(L):
    import ctypes
    import torch
    from blackbox_mpc_amd.engine import Engine
    S, U, A, K = 3, 1, 2, 3
    eng, _, _, _ = _cem(L, PEND_SPEC, A, H5)
    states = _start(A, S)
    acts, sts = np.zeros((K, A, H5, U), F), np.zeros((K, A, H5, S), F)
    d_states = torch.from_numpy(states).cuda()
    d_acts, d_sts = torch.zeros((K, A, H5, U), device="cuda"), torch.zeros((K, A, H5, S), device="cuda")
    vp = ctypes.c_void_p

    def assert_all_state_errors(e):
        count, std = ctypes.c_int32(-7), ctypes.c_float(-7.0)
        assert L.lib.bbmpc_get_policy_prior(e._h, ctypes.byref(count), ctypes.byref(std)) == L.E_STATE
        assert count.value == 0                                 # the count comes back 0 beside the status
        assert L.lib.bbmpc_predict_policy_rollouts(e._h, L.ptr(states), None, L.ptr(acts), L.ptr(sts)) == L.E_STATE
        assert L.lib.bbmpc_predict_policy_rollouts_dev(e._h, vp(d_states.data_ptr()), None, vp(d_acts.data_ptr()),
                                                       vp(d_sts.data_ptr())) == L.E_STATE
        assert L.lib.bbmpc_evaluate_policy_prior(e._h, L.ptr(states), A, L.ptr(np.zeros((A, U), F))) == L.E_STATE
        assert L.lib.bbmpc_evaluate_policy_prior_dev(e._h, vp(d_states.data_ptr()), A, vp(d_acts.data_ptr())) == L.E_STATE
        torch.cuda.synchronize()
        assert not np.any(acts) and not np.any(sts) and not bool(d_acts.any()) and not bool(d_sts.any())     # nothing was written
    assert_all_state_errors(eng)
    assert np.all(np.isfinite(eng.optimize(states)[0]))         # the handle is usable ...
    pol = PP.small_policies(S, U)[1]
    pol.install(eng, K, 0.2)                                    # ... takes a network, and the same calls then succeed
    count, std = ctypes.c_int32(0), ctypes.c_float(0.0)
    assert L.lib.bbmpc_get_policy_prior(eng._h, ctypes.byref(count), ctypes.byref(std)) == 0 and count.value == K
    want = eng.predict_policy_rollouts(states)
    assert L.lib.bbmpc_predict_policy_rollouts_dev(eng._h, vp(d_states.data_ptr()), None, vp(d_acts.data_ptr()), vp(d_sts.data_ptr())) == 0
    eng.synchronize()
    np.testing.assert_array_equal(d_acts.cpu().numpy(), want[0])
    np.testing.assert_array_equal(d_sts.cpu().numpy(), want[1])
    eng.set_policy_prior_mlp(None, None, None)                  # removed: state errors again
    d_acts.zero_()
    d_sts.zero_()
    assert_all_state_errors(eng)
    # a network but no model yet (bbmpc_set_mlp not called): the rollouts are a state error, pi on rows is not
    bare = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_PENDULUM, [-1.0], [1.0], dim_s=S, num_agents=A, planning_horizon=H5,
                  population_size=N, max_iterations=ITERS, num_elite=K_EL)
    pol.install(bare, K, 0.2)
    assert L.lib.bbmpc_predict_policy_rollouts(bare._h, L.ptr(states), None, L.ptr(acts), L.ptr(sts)) == L.E_STATE
    assert L.lib.bbmpc_predict_policy_rollouts_dev(bare._h, vp(d_states.data_ptr()), None, vp(d_acts.data_ptr()),
                                                   vp(d_sts.data_ptr())) == L.E_STATE
    assert "bbmpc_set_mlp" in L.lib.bbmpc_last_error().decode()
    np.testing.assert_allclose(bare.evaluate_policy_prior(states), pol(states), rtol=R.ONE_STEP[0], atol=R.ONE_STEP[1])
    bare.set_mlp(*_dynamics(S, U, [24]))
    assert np.all(np.isfinite(bare.predict_policy_rollouts(states)[0]))


@pytest.mark.parametrize("opt_name", ["OPT_RANDOM_SEARCH", "OPT_PI2", "OPT_PSO", "OPT_SPSA", "OPT_CMAES"])
def test_other_optimizers_are_refused(L, opt_name):
    dims, acts, S, U, reward = PEND_SPEC
    eng = _problem(L, dims, acts, S, U, reward, True, A=1, H=H5, opt=getattr(L, opt_name), N=N, iters=2, k=K_EL)[0]
    pol = PP.small_policies(S, U)[1]
    assert "CEM" in _raises(L, L.E_UNSUPPORTED, lambda: pol.install(eng, 3, 0.1))
    assert _raises(L, L.E_STATE, eng.policy_prior)
    eng.set_policy_prior_mlp(None, None, None)
    assert np.all(np.isfinite(eng.optimize(_start(1, S))[0]))


def test_unsupported_configurations_are_refused_in_both_orders(L, monkeypatch):
    from blackbox_mpc_amd.engine import Engine
    S, U = 3, 1
    pol = PP.small_policies(S, U)[1]
    states = _start(1, S)
    # dynamics other than BBMPC_DYN_MLP
    pend = Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=H5,
                  population_size=N, max_iterations=2, num_elite=K_EL)
    assert "BBMPC_DYN_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: pol.install(pend, 3, 0.1))
    assert np.all(np.isfinite(pend.optimize(O.pendulum_start_states(1))[0]))
    # an inverse target transform, both orders
    xform = "__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {\n" \
            "    for (int i = 0; i < S; ++i) next[i] = dev[i] + cur[i];\n}\n"
    eng, _, _, _ = _cem(L, PEND_SPEC, 1, H5)
    pol.install(eng, 3, 0.1)
    ref = eng.predict_policy_rollouts(states)
    assert "policy prior" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_inverse_transform_source(xform))
    # a model ensemble and log-variance heads behind the prior
    ws, bs = O.make_mlp_params(PEND_SPEC[0], seed=9)
    assert "policy prior" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_mlp_ensemble([(ws, bs), (ws, bs)]))
    hw, hb = np.zeros((PEND_SPEC[0][-2], S), F), np.zeros(S, F)
    assert "policy prior" in _raises(L, L.E_UNSUPPORTED,
                                     lambda: eng.set_mlp_logvar_head([(hw, hb)], np.full(S, -5.0, F), np.full(S, 1.0, F)))
    for x, y in zip(ref, eng.predict_policy_rollouts(states)):             # the handle is usable and unchanged
        np.testing.assert_array_equal(x, y)
    assert eng.policy_prior() == (3, pytest.approx(0.1))
    # ... and the prior behind them
    e2, _, _, _ = _cem(L, PEND_SPEC, 1, H5)
    e2.set_inverse_transform_source(xform)
    assert "transform" in _raises(L, L.E_UNSUPPORTED, lambda: pol.install(e2, 3, 0.1))
    e3, _, _, _ = _cem(L, PEND_SPEC, 1, H5)
    e3.set_mlp_ensemble([(ws, bs), (ws, bs)])
    assert "ensemble" in _raises(L, L.E_UNSUPPORTED, lambda: pol.install(e3, 3, 0.1))
    e3.set_mlp_ensemble([])
    e3.set_mlp_logvar_head([(hw, hb)], np.full(S, -5.0, F), np.full(S, 1.0, F))
    assert "log-variance" in _raises(L, L.E_UNSUPPORTED, lambda: pol.install(e3, 3, 0.1))
    assert _raises(L, L.E_STATE, e3.policy_prior)
    assert np.all(np.isfinite(e3.optimize(states)[0]))
    # a sharded population
    monkeypatch.setenv("BBMPC_POPSHARD_LOOPBACK", "2")
    e4, _, _, _ = _cem(L, PEND_SPEC, 1, H5)
    assert "sharded" in _raises(L, L.E_UNSUPPORTED, lambda: pol.install(e4, 3, 0.1))
    assert np.all(np.isfinite(e4.optimize(states)[0]))


def test_callback_plug_ins_are_refused_in_both_orders(L):
    from blackbox_mpc_amd.engine import Engine
    S, U = 3, 1
    pol = PP.small_policies(S, U)[1]

    def make():
        eng = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_USER, [-1.0], [1.0], dim_s=S, num_agents=1, planning_horizon=H5,
                     population_size=N, max_iterations=2, num_elite=K_EL)
        eng.set_mlp(*_dynamics(S, U, [24]))
        return eng
    cb = L.ROWS_CALLBACK(lambda *a: 0)
    eng = make()
    assert L.lib.bbmpc_set_reward_callback(eng._h, cb, None) == 0
    assert "callback" in _raises(L, L.E_UNSUPPORTED, lambda: pol.install(eng, 3, 0.1))
    eng = make()
    pol.install(eng, 3, 0.1)
    assert L.lib.bbmpc_set_reward_callback(eng._h, cb, None) == L.E_UNSUPPORTED
    assert eng.policy_prior() == (3, pytest.approx(0.1))


# ---- 9. the Python surface -------------------------------------------------------------------------------------------------
def test_mpc_policy_end_to_end_with_a_fitted_linear_policy(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.policies import MPCPolicy, RandomPolicy
    from blackbox_mpc_amd.policy_functions import LearnedPolicyMLP
    from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.dynamics_learning import learn_dynamics_from_policy
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function
    from blackbox_mpc_amd.utils.rollouts import ModelEnvironment
    act, obs = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    rng = np.random.default_rng(0)
    gain = np.array([[0.4], [-0.9], [-0.25]], F)                # a known linear feedback law, inside the bounds on these states
    x = rng.uniform([-1, -1, -2], [1, 1, 2], (800, 3)).astype(F)
    pi = LearnedPolicyMLP(3, 1, [1], [None], seed=1)
    pi.train(x, x @ gain, epochs=60, batch_size=64, learning_rate=2e-2, device="cpu", seed=0)
    assert np.max(np.abs(pi(x) - x @ gain)) < 0.05
    K, A, H = 3, 2, 5
    states = O.pendulum_start_states(A)
    # a learned model, and a second policy network cloned from the executed actions of the collected rollouts
    true_handler = SystemDynamicsHandler(act, obs, dynamics_function=PendulumTrueModel(), true_model=True)
    env = ModelEnvironment(DeterministicTrajectoryEvaluator(pendulum_reward_function, true_handler), states)
    cloned = LearnedPolicyMLP(3, 1, [8, 1], ["tanh", None], seed=2)
    handler = learn_dynamics_from_policy(
        env, RandomPolicy(A, act, seed=0), number_of_rollouts=2, task_horizon=20,
        dynamics_function=DeterministicMLP(layers=[4, 16, 3], activation_functions=["tanh", None], seed=0), epochs=2, batch_size=32, seed=0,
        policy_model=cloned, policy_train_args=dict(epochs=2, batch_size=32, seed=0, device="cpu"))
    assert cloned._version > 0 and cloned.normalization_stats() is not None and len(cloned._pairs) == 2
    assert cloned._pairs[0][0].shape == (20 * A, 3) and cloned._pairs[0][1].shape == (20 * A, 1)
    pol = MPCPolicy(optimizer_name="CEM", policy_prior=pi, prior_candidates=K, prior_std=0.0, reward_function=pendulum_reward_function,
                    env_action_space=act, env_observation_space=obs, dynamics_handler=handler,
                    num_agents=A, planning_horizon=H, population_size=N, max_iterations=ITERS, num_elite=K_EL, seed=9)
    eng = pol._optimizer._engine
    assert eng.policy_prior() == (K, 0.0)
    eng.set_trace(True)
    action, nxt, _ = pol.act(states, 0)
    assert action.shape == (A, 1) and np.all(np.isfinite(action)) and np.all(np.abs(action) <= 2.0)
    cols = eng.get_trace(0, L.TRACE_SAMPLES)[N - K:]
    # the traced columns are the policy's closed-loop rollouts: the first action is the feedback law at the start state, and
    # every column is the rollout bbmpc_predict_policy_rollouts returns (sigma = 0: the K columns are equal)
    np.testing.assert_allclose(cols[:, :, 0], np.broadcast_to(pi(states)[None], (K, A, 1)), rtol=R.ONE_STEP[0], atol=R.ONE_STEP[1])
    np.testing.assert_array_equal(cols, eng.predict_policy_rollouts(states, want_states=False)[0])
    np.testing.assert_array_equal(cols[0], cols[K - 1])
    # a refit bumps the version: the optimizer uploads the network again before its next computation
    pi.train(x, -(x @ gain), epochs=60, batch_size=64, learning_rate=2e-2, device="cpu", seed=0)
    pol.act(states, 1)
    cols2 = eng.get_trace(0, L.TRACE_SAMPLES)[N - K:]
    np.testing.assert_allclose(cols2[:, :, 0], np.broadcast_to(pi(states)[None], (K, A, 1)), rtol=R.ONE_STEP[0], atol=R.ONE_STEP[1])
    assert not np.allclose(cols2[:, :, 0], cols[:, :, 0], atol=1e-3)
    with pytest.raises(TypeError):
        MPCPolicy(optimizer_name="PI2", policy_prior=pi, prior_candidates=K, reward_function=pendulum_reward_function,
                  env_action_space=act, env_observation_space=obs, dynamics_handler=handler,
                  num_agents=A, planning_horizon=H, population_size=N, max_iterations=ITERS)
